"""CPU checks of ReferenceLoss (deep_learning_parameters.py:170-196) on the device: the C ABI of its entry points without a
GPU, the workspace size, the fixture's coverage (tests/golden/refloss.npz), the torch formulas the backward kernels follow,
and the inputs ReferenceLoss hands to torch's own l1_loss / mse_loss."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch

import underwater_image_enhancement_amd as uw
from underwater_image_enhancement_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refloss.npz")
NEW = ("uwie_ref_loss_f32", "uwie_ref_loss_bwd_f32", "uwie_ref_loss_workspace_bytes", "uwie_device_status_async")
E_INVALID = -1
FAKE = ctypes.c_void_p(16)  # never dereferenced: every check below fails before the device guard


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return uw.load()


def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    tags = sorted({k.split("/")[0] for k in d})
    return {t: {k.split("/", 1)[1]: v for k, v in d.items() if k.startswith(t + "/")} for t in tags}


def test_symbols_are_exported_and_bound(lib):
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
    assert (_lib.LOSS_IDENTITY, _lib.LOSS_VGG, _lib.LOSS_GATED) == (0, 1, 2)
    for name in ("ReferenceLoss", "RefLossFunction", "DiffEnhanceLossFunction", "GatedDiffEnhanceLossFunction"):
        assert name in uw.__all__ and hasattr(uw, name), name
    assert callable(uw.DifferentiableEnhancement.with_loss) and callable(uw.GatedDifferentiableEnhancement.with_loss)


def fwd(lib, ctx=FAKE, map_=0, img=FAKE, params=None, flags=0, B=1, H=8, W=8, ref=FAKE, out=None, saved=None, loss=FAKE,
        ws=None, nbytes=0):
    return lib.uwie_ref_loss_f32(ctx, map_, img, params, flags, 1, B, H, W, ref, out, saved, loss, ws, nbytes, None)


def bwd(lib, ctx=FAKE, map_=0, img=FAKE, params=None, flags=0, B=1, H=8, W=8, saved=None, ref=FAKE, gout=None, gl=FAKE,
        gimg=ctypes.c_void_p(32), gparams=None, ws=None, nbytes=0):
    return lib.uwie_ref_loss_bwd_f32(ctx, map_, img, params, flags, 1, B, H, W, saved, ref, gout, gl, gimg, gparams, ws, nbytes,
                                     None)


def test_entry_points_reject_null_arguments_without_a_gpu(lib):
    for kw in ({"ctx": None}, {"img": None}, {"ref": None}, {"loss": None}, {"map_": 1}, {"map_": 2, "params": FAKE}):
        assert fwd(lib, **kw) == E_INVALID, kw
        assert b"NULL" in lib.uwie_last_error(), kw
    for kw in ({"ctx": None}, {"img": None}, {"ref": None}, {"gl": None}, {"gimg": None}, {"map_": 1, "params": FAKE, "saved": FAKE},
               {"map_": 2}):
        assert bwd(lib, **kw) == E_INVALID, kw
        assert b"NULL" in lib.uwie_last_error(), kw
    assert lib.uwie_device_status_async(None, FAKE, None) == E_INVALID


def test_entry_points_reject_shapes_maps_and_flags_without_a_gpu(lib):
    for kw in ({"B": 0}, {"H": 0}, {"W": -3}, {"H": 1 << 15, "W": 1 << 15}):
        assert fwd(lib, **kw) == E_INVALID, kw
        assert b"out of range" in lib.uwie_last_error(), kw
        assert bwd(lib, **kw) == E_INVALID, kw
    assert fwd(lib, map_=3) == E_INVALID and b"map" in lib.uwie_last_error()
    assert bwd(lib, map_=-1) == E_INVALID and b"map" in lib.uwie_last_error()
    assert fwd(lib, map_=1, params=FAKE, saved=FAKE, flags=4) == E_INVALID and b"flags" in lib.uwie_last_error()
    assert fwd(lib, map_=2, params=FAKE, saved=FAKE, flags=1) == E_INVALID and b"flags" in lib.uwie_last_error()
    assert bwd(lib, gimg=FAKE) == E_INVALID and b"alias" in lib.uwie_last_error()
    assert bwd(lib, gimg=ctypes.c_void_p(48), gout=ctypes.c_void_p(48)) == E_INVALID and b"alias" in lib.uwie_last_error()
    # a vgg / gated call without workspace: refused before any launch
    assert fwd(lib, map_=2, params=FAKE, saved=FAKE) != 0 and b"workspace" in lib.uwie_last_error()


def test_workspace_sizes(lib):
    for B, H, W in ((1, 1, 1), (4, 256, 256), (32, 224, 224), (8, 2160, 3840), (2, 1080, 1920), (3, 211, 157)):
        need = lib.uwie_ref_loss_workspace_bytes(B, H, W)
        assert need >= lib.uwie_diff_enhance_bwd_workspace_bytes(B, H, W)
        n = H * W
        gx = min(-(-n // 2048), 512)
        chunk = (-(-n // gx) + 255) & ~255
        gx = -(-n // chunk)
        assert need >= 16 * B * gx, (B, H, W)  # two float64 partials per block
        assert need % 256 == 0
        assert need <= lib.uwie_workspace_bytes(B, H, W, None) + 16 * B * 512 + 512
    for bad in ((0, 8, 8), (1, 0, 8), (1, 8, -1)):
        assert lib.uwie_ref_loss_workspace_bytes(*bad) == 0


CASES = ("gated_u8ties_2x3x24x31", "gated_use0_2x3x13x19", "gated_use1_2x3x11x23", "gated_usemix_4x3x10x9",
         "gated_equal_2x3x12x15", "gated_nanref_2x3x9x14", "vgg_u8ties_2x3x20x27", "vgg_omega_equal_2x3x14x17",
         "vgg_gamma_3x3x9x21", "vgg_stretch_1x3x16x16")


def test_the_fixture_covers_its_cases():
    g = golden()
    assert tuple(sorted(g)) == tuple(sorted(CASES))
    assert os.path.getsize(GOLDEN) < 400_000
    weights = {tuple(np.asarray(c["w"]).tolist()) for c in g.values()}
    assert {(0.5, 0.5), (np.float32(0.3).item(), 0.5)} <= weights
    kinds = {int(c["kind"]) for c in g.values()}
    assert kinds == {0, 1}
    u = np.concatenate([c["use_gamma"].ravel() for c in g.values() if int(c["kind"]) == 0])
    assert (u == 0).any() and (u == 1).any() and ((u > 0) & (u < 1)).any()
    # the sgn(0) rule: references equal to the output somewhere; a NaN reference gives NaN losses and NaN parameter grads
    assert any(np.count_nonzero(c["grad_out"] * c["w"][1] == 0) > 0 for t, c in g.items() if "equal" in t)
    nan = g["gated_nanref_2x3x9x14"]
    assert np.isnan(nan["ref"]).sum() == 1 and np.isnan(nan["l1"]) and np.isnan(nan["l2"])
    assert np.isnan(nan["grad_gamma"][1]) and np.isfinite(nan["grad_gamma"][0])
    u8 = g["gated_u8ties_2x3x24x31"]["img"]
    assert len(np.unique(u8)) <= 16
    for t, c in g.items():
        if "nan" in t:
            continue
        assert np.isfinite(c["l1"]) and np.isfinite(c["l2"]) and np.isfinite(c["grad_img_stable"]).all(), t
        assert c["total"] == np.float32(c["w"][0]) * c["l1"] + np.float32(c["w"][1]) * c["l2"] or \
            abs(float(c["total"]) - (float(c["w"][0]) * float(c["l1"]) + float(c["w"][1]) * float(c["l2"]))) < 1e-6, t


def loss_grad_np(o, r, g1, g2):
    """The formula the backward kernels evaluate (k_diffenh.hip refloss_grad), in float32 NumPy."""
    N = o.size
    d = o - r
    sg = np.sign(d).astype(np.float32)
    sg[np.isnan(d)] = 0.0
    return (np.float32(g1) / np.float32(N)) * sg + (np.float32(2.0 / N) * d) * np.float32(g2)


@pytest.mark.parametrize("shape", [(2, 3, 17, 19), (1, 3, 64, 80), (4, 3, 33, 7)])
@pytest.mark.parametrize("w1,w2,up", [(0.5, 0.5, 1.0), (0.3, 0.5, 1.0), (0.5, 0.5, 3.7), (1.3, 0.7, -2.1)])
def test_the_kernel_formula_is_torch_cpu_autograd_bit_for_bit(shape, w1, w2, up):
    """Pins torch's operation order (MeanBackward0 -> AbsBackward0, MseLossBackward0, their sum) in the installed torch."""
    rng = np.random.default_rng(sum(shape))
    o = rng.random(shape, dtype=np.float32)
    r = rng.random(shape, dtype=np.float32)
    r.reshape(-1)[::5] = o.reshape(-1)[::5]  # sgn(0) = 0
    ot = torch.from_numpy(o.copy()).requires_grad_(True)
    l1 = torch.nn.functional.l1_loss(ot, torch.from_numpy(r))
    l2 = torch.nn.functional.mse_loss(ot, torch.from_numpy(r))
    (up * (w1 * l1 + w2 * l2)).backward()
    g1 = np.float32(up) * np.float32(w1)
    g2 = np.float32(up) * np.float32(w2)
    want = ot.grad.numpy()
    got = loss_grad_np(o, r, g1, g2)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    # the values: float64 sums of the float32 terms, rounded once, within 1e-6 of torch CPU's own result
    d = o - r
    assert abs(np.float32(np.abs(d).astype(np.float64).sum() / d.size) - l1.item()) <= 1e-6 * l1.item()
    assert abs(np.float32((d * d).astype(np.float64).sum() / d.size) - l2.item()) <= 1e-6 * l2.item()


def reference_loss(enhanced, reference, w1, w2):
    l1 = torch.nn.L1Loss()(enhanced, reference)
    l2 = torch.nn.MSELoss()(enhanced, reference)
    return w1 * l1 + w2 * l2, {"l1": l1.item(), "l2": l2.item()}


def test_reference_loss_on_cpu_tensors_is_torch():
    rng = np.random.default_rng(3)
    o = torch.from_numpy(rng.random((2, 3, 9, 11), dtype=np.float32)).requires_grad_(True)
    r = torch.from_numpy(rng.random((2, 3, 9, 11), dtype=np.float32))
    loss, parts = uw.ReferenceLoss(0.3, 0.5)(o, r)
    o2 = o.detach().clone().requires_grad_(True)
    want, wparts = reference_loss(o2, r, 0.3, 0.5)
    assert parts == wparts and torch.equal(loss, want)
    loss.backward()
    want.backward()
    assert torch.equal(o.grad, o2.grad)
    assert isinstance(uw.ReferenceLoss(), torch.nn.Module)


def test_reference_loss_other_dtypes_are_torch():
    rng = np.random.default_rng(4)
    o = torch.from_numpy(rng.random((1, 3, 5, 6)))  # float64
    r = torch.from_numpy(rng.random((1, 3, 5, 6)))
    loss, parts = uw.ReferenceLoss()(o, r)
    want, wparts = reference_loss(o, r, 0.5, 0.5)
    assert loss.dtype == torch.float64 and parts == wparts and torch.equal(loss, want)


def test_reference_loss_broadcasts_with_torchs_warning():
    rng = np.random.default_rng(5)
    o = torch.from_numpy(rng.random((2, 3, 4, 5), dtype=np.float32))
    r = torch.from_numpy(rng.random((1, 3, 4, 5), dtype=np.float32))
    with pytest.warns(UserWarning, match="target size"):
        loss, parts = uw.ReferenceLoss()(o, r)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want, wparts = reference_loss(o, r, 0.5, 0.5)
    assert parts == wparts and torch.equal(loss, want)
