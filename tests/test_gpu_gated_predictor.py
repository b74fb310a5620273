"""ParameterPredictor on the device (uwie_mlp_*, uw.ParameterPredictor) and uw.GatedEnhancementPredictor (DESIGN.md section
17): the MLP against the real module's goldens and the float64 evaluation (tests/gated_predictor_ref.py) within
R.DEVICE_TOL of each head's range -- the measured float32-against-float64 difference of the real module times a stated
margin, tests/test_gated_predictor_ref.py -- and the predictor's routes against each other."""
import os

import numpy as np
import pytest

import gated_predictor_ref as R
import param_net_ref as PN

pytestmark = pytest.mark.gpu

PN_GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "param_net.npz")


@pytest.fixture(scope="module")
def dev():
    import underwater_image_enhancement_amd as uw

    return uw.get_device(0)


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


@pytest.fixture(scope="module")
def nets(gold):
    """name -> (state, uw.ParameterPredictor)"""
    import underwater_image_enhancement_amd as uw

    big, small = R.seeded_state(int(gold["seed"])), R.small_state(gold)
    return {"big": (big, uw.ParameterPredictor(big)), "small": (small, uw.ParameterPredictor(small))}


def host(params):
    return {k: v.cpu().numpy() for k, v in params.items()}


def test_against_the_goldens(dev, gold, nets):
    import torch

    for net, tags in (("big", ("unit", "large", "one")), ("small", ("small",))):
        state, model = nets[net]
        assert (model.feature_dim, model.hidden_dim, model.num_blocks) == ((79, 256, 3) if net == "big" else (79, 64, 1))
        for tag in tags:
            rows = gold[f"{tag}/rows"]
            got = model(rows)  # float64 rows, rounded on load
            assert list(got) == list(R.HEADS)
            assert all(v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (rows.shape[0], 1) for v in got.values())
            got = host(got)
            e_gold = R.worst_fraction(got, {k: gold[f"{tag}/{k}"] for k in R.HEADS})
            e_f64 = R.worst_fraction(got, R.forward64(state, rows))
            print(f"{tag}: {e_gold:.3g} of the range from the real module, {e_f64:.3g} from float64 (tolerance {R.DEVICE_TOL:.3g})")
            assert e_gold <= R.DEVICE_TOL and e_f64 <= R.DEVICE_TOL, tag
            # float32 rows are the float64 rows rounded: the same bits
            again = host(model(rows.astype(np.float32)))
            assert all(np.array_equal(again[k].view(np.int32), got[k].view(np.int32)) for k in R.HEADS), tag


@pytest.mark.parametrize("net", ["big", "small"])
def test_rows_do_not_depend_on_the_batch(dev, nets, net):
    state, model = nets[net]
    rows = np.random.default_rng(7).standard_normal((70, 79)) * 2.0  # 70 rows: three LDS staging passes at hidden = 256
    whole = model.columns(rows)
    assert tuple(whole.shape) == (70, 4)
    w = whole.cpu().numpy()
    want = R.columns(R.forward64(state, rows))
    span = np.array([R.SPAN[k] for k in R.GATED_ORDER])
    err = float((np.abs(w - want) / span).max())
    print(f"{net}: B = 70, {err:.3g} of the range from float64")
    assert err <= R.DEVICE_TOL
    for B in (1, 3):
        part = model.columns(rows[:B]).cpu().numpy()
        assert np.array_equal(part.view(np.int32), w[:B].view(np.int32)), B
    last = model.columns(rows[69:]).cpu().numpy()
    assert np.array_equal(last.view(np.int32), w[69:].view(np.int32))
    assert np.array_equal(model.columns(rows).cpu().numpy().view(np.int32), w.view(np.int32))  # repeatable


def test_every_form_of_state(dev, gold, nets, tmp_path):
    import torch

    import underwater_image_enhancement_amd as uw

    state, model = nets["small"]
    rows = gold["small/rows"]
    want = model.columns(rows).cpu().numpy().view(np.int32)
    tensors = {k: torch.from_numpy(v) for k, v in state.items()}

    class Block(torch.nn.Module):
        def __init__(self, dim):
            super().__init__()
            self.block = torch.nn.Sequential(torch.nn.Linear(dim, dim), torch.nn.ReLU(), torch.nn.Dropout(0.3), torch.nn.Linear(dim, dim))

    class Net(torch.nn.Module):  # a module with the reference's state-dict keys
        def __init__(self):
            super().__init__()
            self.input_proj = torch.nn.Sequential(torch.nn.Linear(79, 64), torch.nn.ReLU(), torch.nn.Dropout(0.3))
            self.res_blocks = torch.nn.ModuleList([Block(64)])
            self.output_proj = torch.nn.Sequential(torch.nn.Linear(64, 32), torch.nn.ReLU())
            self.param_heads = torch.nn.ModuleDict({k: torch.nn.Linear(32, 1) for k in R.HEADS})

    module = Net()
    assert list(module.state_dict()) == list(state)
    module.load_state_dict(tensors)
    ckpt = {"param_predictor": tensors, "optimizer": {"state": {}, "param_groups": []}}
    path = tmp_path / "best_model.pth"
    torch.save(ckpt, path)
    for form in (tensors, module, ckpt, str(path), path):
        p = uw.ParameterPredictor(form)
        assert (p.feature_dim, p.hidden_dim, p.num_blocks) == (79, 64, 1)
        assert np.array_equal(p.columns(rows).cpu().numpy().view(np.int32), want), type(form)
        p.close()
    # a state that is not this module's: the vgg network's
    with pytest.raises(ValueError, match="input_proj.0.weight"):
        uw.ParameterPredictor(PN.seeded_state(int(np.load(PN_GOLD, allow_pickle=False)["seed"])))
    bad = dict(tensors)
    bad["res_blocks.0.block.3.weight"] = torch.zeros(64, 63)
    with pytest.raises(ValueError, match="res_blocks.0.block.3.weight"):
        uw.ParameterPredictor(bad)
    bad = {k: v for k, v in tensors.items() if k != "param_heads.L_high.bias"}
    with pytest.raises(ValueError, match="param_heads.L_high.bias"):
        uw.ParameterPredictor(bad)
    with pytest.raises(RuntimeError):
        model(rows[:, :74])


@pytest.fixture(scope="module")
def predictor(gold):
    import underwater_image_enhancement_amd as uw

    return uw.GatedEnhancementPredictor(R.seeded_state(int(gold["seed"])))


def test_enhance_batch_u8(dev, predictor):
    import torch

    frames = np.random.default_rng(21).integers(0, 256, (3, 40, 56, 3), dtype=np.uint8)
    out, params = predictor.enhance_batch_u8(frames)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (3, 40, 56, 3)
    assert params.is_cuda and params.dtype == torch.float32 and tuple(params.shape) == (3, 4)
    f = predictor.enhance_batch(frames)
    assert f.is_cuda and f.dtype == torch.float32 and tuple(f.shape) == (3, 40, 56, 3)
    assert np.array_equal(out.cpu().numpy(), (f * 255).to(torch.uint8).cpu().numpy())
    assert dev.check_status() == 0
    pp = predictor.predict_parameters(frames)
    assert list(pp) == list(R.HEADS)
    cols = params.cpu().numpy()
    for i, k in enumerate(R.GATED_ORDER):
        assert pp[k].dtype == np.float64 and np.array_equal(pp[k], cols[:, i].astype(np.float64)), k
    one = predictor.predict_parameters(frames[1])
    assert all(type(v) is float for v in one.values()) and one == {k: float(pp[k][1]) for k in R.HEADS}
    # the network's rows are FeatureExtractor's
    rows = dev.feature_extractor(dev.tensor(frames))
    assert np.array_equal(predictor.model.columns(rows).cpu().numpy().view(np.int32), cols.view(np.int32))
    # the float forms of the same frames
    for x in (dev.tensor(frames), frames.astype(np.float32) / np.float32(255.0), frames / 255):
        again, p = predictor.enhance_batch_u8(x)
        assert np.array_equal(again.cpu().numpy(), out.cpu().numpy()) and np.array_equal(p.cpu().numpy(), cols)


def test_process_frames(dev, predictor):
    rng = np.random.default_rng(22)
    sizes = [(40, 56), (24, 32), (40, 56), (18, 10), (24, 32), (40, 56)]
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    frames.insert(3, rng.integers(0, 256, (24, 32, 3)).astype(np.int32))  # a frame the predictor does not take
    names = [f"frame{i}.png" for i in range(len(frames))]
    outs, params = predictor.process_frames(frames, names)
    assert len(outs) == len(params) == len(frames)
    for i, f in enumerate(frames):
        if i == 3:
            assert outs[i] is None and isinstance(params[i], str) and params[i].startswith("frame3.png: ") and "int32" in params[i]
            continue
        one, _ = predictor.enhance_batch_u8(f)
        assert isinstance(outs[i], np.ndarray) and outs[i].dtype == np.uint8 and outs[i].shape == frames[i].shape
        assert np.array_equal(outs[i], one.cpu().numpy()[0]), i
        want = predictor.predict_parameters(f)
        assert params[i] == want and list(params[i]) == list(want) and all(type(v) is float for v in params[i].values()), i
    plain, msgs = predictor.process_frames(frames[3:4])
    assert plain == [None] and "int32" in msgs[0] and not msgs[0].startswith("frame")
    with pytest.raises(ValueError):
        predictor.process_frames(frames, names[:2])
    assert predictor.process_frames([]) == ([], [])


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-30)


def test_validate_batch(dev, gold):
    import torch

    import underwater_image_enhancement_amd as uw

    predictor = uw.GatedEnhancementPredictor(R.small_state(gold))
    total, parts_sum = 0.0, {"l1": 0.0, "l2": 0.0}
    for i in range(2):
        img, ref, feat = (gold[f"validate/{i}/{k}"] for k in ("image", "reference", "features"))
        loss, parts = predictor.validate_batch(dev.tensor(img), dev.tensor(ref), dev.tensor(feat))
        assert isinstance(loss, torch.Tensor) and loss.dim() == 0 and not loss.requires_grad
        assert sorted(parts) == ["l1", "l2"] and all(type(v) is float for v in parts.values())
        # ReferenceLoss's tolerances against the reference's values (tests/test_gpu_refloss.py)
        assert rel(parts["l1"], float(gold[f"validate/{i}/l1"])) <= 1e-5 and rel(parts["l2"], float(gold[f"validate/{i}/l2"])) <= 1e-5
        assert rel(loss.item(), float(gold[f"validate/{i}/loss"])) <= 2e-5
        total += loss.item()
        for k in parts_sum:
            parts_sum[k] += parts[k]
        again, p2 = predictor.validate_batch(img, ref, feat)  # NumPy batches
        assert again.item() == loss.item() and p2 == parts
    # EndToEndTrainer.validate's averages
    assert rel(total / 2, float(gold["validate/loss"])) <= 2e-5
    assert rel(parts_sum["l1"] / 2, float(gold["validate/l1"])) <= 1e-5 and rel(parts_sum["l2"] / 2, float(gold["validate/l2"])) <= 1e-5
    # features=None: FeatureExtractor's rows of the images
    img, ref = gold["validate/0/image"], gold["validate/0/reference"]
    loss, parts = predictor.validate_batch(img, ref)
    u8 = (img.transpose(0, 2, 3, 1) * 255).astype(np.uint8)
    rows = dev.feature_extractor(dev.tensor(u8))
    want, wparts = predictor.validate_batch(img, ref, rows)
    assert loss.item() == want.item() and parts == wparts
