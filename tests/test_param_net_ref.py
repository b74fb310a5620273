"""ImprovedVGGParameterNet without a GPU: the float64 restatement (tests/param_net_ref.py) and the
torch route against the golden of the real module (tests/golden/param_net.npz), state-dict validation, and the C ABI's
symbols, parameter counts and workspace formula."""
import math
import os

import numpy as np
import pytest
import torch

import param_net_ref as PN

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "param_net.npz")


def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    tags = sorted({k.split("/")[0] for k in d if "/" in k})
    return d, {t: {k.split("/", 1)[1]: v for k, v in d.items() if k.startswith(t + "/")} for t in tags}


@pytest.fixture(scope="module")
def state():
    d, _ = golden()
    return PN.seeded_state(int(d["seed"]))


def test_seeded_weights_are_the_goldens():
    d, _ = golden()
    seed = int(d["seed"])
    assert PN.checksum(PN.seeded_state(seed)) == float(d["checksum"])
    assert PN.checksum(PN.seeded_state(seed, False), False) == float(d["checksum_nofeat"])


def test_restatement_reproduces_the_reference_golden():
    """The float64 restatement gives the real module's pooled vector and parameters within 1e-6 (relative to max |pooled|
    and to each parameter's range)."""
    d, cases = golden()
    seed = int(d["seed"])
    for tag, c in cases.items():
        if tag.startswith("pred_"):
            continue
        uf = bool(c["use_features"])
        pooled, params = PN.forward(PN.seeded_state(seed, uf), c["img"], c.get("features"), uf)
        assert np.array_equal(c["pooled"][:, 512:], c["pooled"][:, :512]), tag  # the reference's "maxpool" quirk
        assert np.abs(pooled - c["pooled"]).max() <= 1e-6 * np.abs(c["pooled"]).max(), tag
        for i, k in enumerate(PN.KEYS):
            lo, hi = PN.RANGES[k]
            assert np.abs(params[:, i] - c["params"][:, i]).max() <= 1e-6 * (hi - lo), (tag, k)


def test_torch_route_reproduces_the_golden():
    import underwater_image_enhancement_amd as uw

    d, cases = golden()
    seed = int(d["seed"])
    for tag, c in cases.items():
        if tag.startswith("pred_"):
            continue
        uf = bool(c["use_features"])
        net = uw.VGGParameterNet(PN.seeded_state(seed, uf), use_features=uf)
        feats = torch.from_numpy(c["features"]) if "features" in c else None
        with torch.no_grad():
            out = net(torch.from_numpy(c["img"]), feats, return_pooled=True)
        assert set(out) == set(PN.KEYS) | {"pooled"}
        for i, k in enumerate(PN.KEYS):
            assert out[k].shape == (c["img"].shape[0], 1) and out[k].dtype == torch.float32
            lo, hi = PN.RANGES[k]
            assert np.abs(out[k].numpy()[:, 0] - c["params"][:, i]).max() <= 1e-6 * (hi - lo), (tag, k)
        assert np.abs(out["pooled"].numpy() - c["pooled"]).max() <= 1e-6 * np.abs(c["pooled"]).max(), tag


def test_layout_matches_the_c_abi_counts():
    import underwater_image_enhancement_amd as uw
    from underwater_image_enhancement_amd import _lib

    for uf in (True, False):
        lay = uw.param_net_layout(uf)
        assert lay == PN.layout(uf)
        assert sum(math.prod(s) for _, s in lay) == _lib.PARAM_NET_PARAMS[uf]
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uwie.h")).read()
    assert "#define UWIE_PARAM_NET_PARAMS(use_features) ((use_features) ? 8500100 : 8459652)" in text


def test_missing_key_and_wrong_shape_name_the_key(state):
    import underwater_image_enhancement_amd as uw

    missing = {k: v for k, v in state.items() if k != "feature_fusion.5.running_var"}
    with pytest.raises(ValueError, match="feature_fusion.5.running_var"):
        uw.VGGParameterNet(missing)
    wrong = dict(state)
    wrong["vgg_features.19.weight"] = np.zeros((512, 256, 3, 3), np.float32)
    with pytest.raises(ValueError, match="vgg_features.19.weight"):
        uw.param_net_torch(wrong)
    with pytest.raises(ValueError, match="feature_fusion.0.weight"):
        uw.VGGParameterNet(state, use_features=False)  # a 1103-input state dict on a 1024-input net


def test_hidden_dim_other_than_256_is_refused(state):
    import underwater_image_enhancement_amd as uw

    with pytest.raises(ValueError, match="hidden_dim"):
        uw.VGGParameterNet(state, hidden_dim=128)
    with pytest.raises(ValueError, match="hidden_dim"):
        uw.param_net_torch(state, hidden_dim=512)


def test_checkpoint_dicts_and_paths_are_unwrapped(state, tmp_path):
    import underwater_image_enhancement_amd as uw

    sd = {k: torch.from_numpy(v) for k, v in state.items()}
    sd["feature_fusion.1.num_batches_tracked"] = torch.tensor(7)
    x = torch.from_numpy(np.random.default_rng(0).standard_normal((2, 3, 16, 16)).astype(np.float32))
    f = torch.from_numpy(np.random.default_rng(1).random((2, 79), dtype=np.float32))
    want = uw.param_net_torch(state)(x, f)
    path = tmp_path / "best_model.pth"
    torch.save({"epoch": 3, "model_state_dict": sd, "optimizer_state_dict": {}}, path)
    for w in (str(path), {"model_state_dict": sd}, sd):
        got = uw.VGGParameterNet(w)(x, f)
        for k in PN.KEYS:
            assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("shape", [(1, 3, 7, 16), (1, 3, 16, 7), (2, 3, 4, 4)])
def test_small_frames_raise_on_the_torch_route(state, shape):
    import underwater_image_enhancement_amd as uw

    with pytest.raises(RuntimeError):
        uw.VGGParameterNet(state)(torch.zeros(shape), torch.zeros((shape[0], 79)))


def test_workspace_formula_and_symbols():
    import underwater_image_enhancement_amd as uw

    lib = uw.load()
    for name in ("uwie_param_net_create", "uwie_param_net_destroy", "uwie_param_net_workspace_bytes", "uwie_param_net_f32"):
        assert hasattr(lib, name), name

    def al(n):
        return (n + 255) // 256 * 256

    for B, H, W in ((1, 224, 224), (2, 20, 27), (3, 8, 8), (32, 224, 224)):
        P = B * H * W
        want = 2 * al(4 * P * 64) + sum(al(4 * B * n) for n in (1103, 512, 256, 64, 256, 512))
        assert lib.uwie_param_net_workspace_bytes(B, H, W) == want, (B, H, W)
    for B, H, W in ((1, 7, 8), (1, 8, 7), (0, 8, 8)):
        assert lib.uwie_param_net_workspace_bytes(B, H, W) == 0


def test_predictor_takes_u8_over_255_in_float32_and_float64():
    """``frame / 255`` (float64, NumPy's default) and ``frame.astype(float32) / 255`` both give the frame back; for every
    byte the reference's ``(img * 255).astype(uint8)`` returns it and the float32 cast equals u8 / 255 in float32."""
    import underwater_image_enhancement_amd as uw

    u = np.arange(256, dtype=np.uint8)
    assert np.array_equal((u / 255 * 255).astype(np.uint8), u)
    assert np.array_equal((u / 255).astype(np.float32), u.astype(np.float32) / np.float32(255.0))
    frame = np.random.default_rng(2).integers(0, 256, (2, 9, 11, 3), dtype=np.uint8)
    for img in (frame / 255, frame.astype(np.float32) / np.float32(255.0), frame[0] / 255, torch.from_numpy(frame / 255)):
        got = uw.EnhancementPredictor._frame_u8(img)
        assert got.dtype == np.uint8 and np.array_equal(got, frame if got.ndim == 4 else frame[0])
    assert uw.EnhancementPredictor._frame_u8(frame) is frame


@pytest.mark.parametrize("img", [np.full((8, 8, 3), 0.5, np.float32), np.full((8, 8, 3), 0.5),
                                 (np.arange(192).reshape(8, 8, 3) / 255).astype(np.float16),
                                 np.full((8, 8, 3), np.nan), np.full((8, 8, 3), 2.0)])
def test_predictor_refuses_float_images_that_are_not_u8_over_255(img):
    import underwater_image_enhancement_amd as uw

    with pytest.raises(uw.UnsupportedInputError):
        uw.EnhancementPredictor._frame_u8(img)
