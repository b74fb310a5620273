"""PerceptualLoss / CombinedLoss without a GPU: the restatement (tests/perceptual_ref.py) and the
torch route against the golden of the real modules (tests/golden/perceptual.npz), weight loading, the small-frame error,
and the torch route on CPU tensors."""
import os

import numpy as np
import pytest
import torch

import perceptual_ref as PR

SEED = 7
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "perceptual.npz")


@pytest.fixture(scope="module")
def state():
    return PR.seeded_weights(SEED)


def golden_cases():
    with np.load(GOLDEN, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    tags = sorted({k.split("/")[0] for k in d if "/" in k})
    return int(d["seed"]), float(d["checksum"]), {t: {k.split("/", 1)[1]: v for k, v in d.items() if k.startswith(t + "/")} for t in tags}


def same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64), equal_nan=True)


def test_restatement_reproduces_the_reference_golden():
    """tests/golden/perceptual.npz comes from the real vgg_16_UIE.PerceptualLoss / CombinedLoss: the restatement gives its
    loss and gradient (float32, torch CPU)."""
    seed, checksum, cases = golden_cases()
    state = PR.seeded_weights(seed)
    assert PR.checksum(state) == checksum, "the seeded weights differ from the ones the golden was made with"
    T = PR.tensors_of(state)
    for tag, c in cases.items():
        loss, grad = PR.loss_and_grad(c["pred"], c["target"], T, "f32")
        if "nan" in tag:
            assert np.isnan(loss) and np.isnan(c["perceptual"])
            continue
        assert abs(float(loss) - float(c["perceptual"])) <= 1e-6 * abs(float(c["perceptual"])), tag
        assert np.abs(grad - c["grad_perceptual"]).max() <= 1e-5 * np.abs(c["grad_perceptual"]).max(), tag


def test_cpu_route_of_combined_loss_reproduces_the_golden():
    import underwater_image_enhancement_amd as uw

    seed, _, cases = golden_cases()
    crit = uw.CombinedLoss(weights=PR.seeded_weights(seed))
    for tag, c in cases.items():
        e = torch.from_numpy(c["pred"].copy()).requires_grad_(True)
        total, parts = crit(e, torch.from_numpy(c["target"]))
        total.backward()
        assert same(parts["l1"], c["l1"]) and same(parts["l2"], c["l2"]), tag
        if "nan" in tag:
            assert np.isnan(parts["perceptual"]) and np.isnan(total.item())
            continue
        assert abs(parts["perceptual"] - float(c["perceptual_part"])) <= 1e-6 * abs(float(c["perceptual_part"])), tag
        assert abs(total.item() - float(c["total"])) <= 1e-6 * abs(float(c["total"])), tag
        assert np.abs(e.grad.numpy() - c["grad_enhanced"]).max() <= 1e-5 * np.abs(c["grad_enhanced"]).max(), tag


def test_weight_key_styles_and_path_load_the_same_module(state, tmp_path):
    import underwater_image_enhancement_amd as uw

    x = torch.from_numpy(np.random.default_rng(0).random((1, 3, 12, 10), dtype=np.float32))
    want = uw.vgg16_features16({k: torch.from_numpy(v) for k, v in state.items()})(x)
    prefixed = {f"features.{k}": torch.from_numpy(v) for k, v in state.items()}
    prefixed["classifier.0.weight"] = torch.zeros(2, 2)  # torchvision's checkpoint holds the classifier too
    assert torch.equal(uw.vgg16_features16(prefixed)(x), want)
    path = tmp_path / "w.pth"
    torch.save(prefixed, path)
    assert torch.equal(uw.vgg16_features16(str(path))(x), want)
    assert want.shape == (1, 256, 3, 2)


def test_bad_weights_name_the_key(state):
    import underwater_image_enhancement_amd as uw

    missing = {k: v for k, v in state.items() if k != "7.bias"}
    with pytest.raises(ValueError, match="7.bias"):
        uw.PerceptualLoss(missing)
    wrong = dict(state)
    wrong["12.weight"] = np.zeros((256, 128, 3, 3), np.float32)
    with pytest.raises(ValueError, match="12.weight"):
        uw.vgg16_features16(wrong)


def test_none_reads_torchvisions_cached_checkpoint_only(state, tmp_path, monkeypatch):
    import underwater_image_enhancement_amd as uw

    monkeypatch.setattr(torch.hub, "get_dir", lambda: str(tmp_path))
    path = os.path.join(str(tmp_path), "checkpoints", "vgg16-397923af.pth")
    with pytest.raises(FileNotFoundError, match="vgg16-397923af.pth"):
        uw.PerceptualLoss()
    os.makedirs(os.path.dirname(path))
    torch.save({f"features.{k}": torch.from_numpy(v) for k, v in state.items()}, path)
    crit = uw.PerceptualLoss()
    x = torch.from_numpy(np.random.default_rng(1).random((1, 3, 8, 9), dtype=np.float32))
    assert torch.equal(crit.features()(x), uw.vgg16_features16(state)(x))


@pytest.mark.parametrize("shape", [(1, 3, 3, 8), (1, 3, 8, 3), (2, 3, 1, 1)])
def test_small_frames_raise(state, shape):
    import underwater_image_enhancement_amd as uw

    with pytest.raises(RuntimeError):
        uw.PerceptualLoss(state)(torch.zeros(shape), torch.zeros(shape))


@pytest.mark.parametrize("shape", [(2, 3, 20, 27), (1, 3, 9, 13), (3, 3, 16, 16)])
def test_cpu_tensors_take_the_torch_route(state, shape):
    import underwater_image_enhancement_amd as uw

    rng = np.random.default_rng(sum(shape))
    pred, target = rng.random(shape, dtype=np.float32), rng.random(shape, dtype=np.float32)
    want_l, want_g = PR.loss_and_grad(pred, target, PR.tensors_of(state), "f32")
    p = torch.from_numpy(pred.copy()).requires_grad_(True)
    loss = uw.PerceptualLoss(state)(p, torch.from_numpy(target))
    loss.backward()
    assert float(loss.detach()) == float(want_l)
    assert np.array_equal(p.grad.double().numpy(), want_g)


def test_combined_loss_cpu_route(state):
    import underwater_image_enhancement_amd as uw

    rng = np.random.default_rng(4)
    e = torch.from_numpy(rng.random((2, 3, 12, 14), dtype=np.float32)).requires_grad_(True)
    r = torch.from_numpy(rng.random((2, 3, 12, 14), dtype=np.float32))
    total, parts = uw.CombinedLoss(weights=state)(e, r)
    vgg = uw.vgg16_features16(state)
    l1, l2 = torch.nn.functional.l1_loss(e, r), torch.nn.functional.mse_loss(e, r)
    p = torch.nn.functional.mse_loss(vgg(e), vgg(r))
    assert parts == {"l1": l1.item(), "l2": l2.item(), "perceptual": p.item()}
    assert total.item() == (0.3 * l1 + 0.5 * l2 + 0.2 * p).item()
