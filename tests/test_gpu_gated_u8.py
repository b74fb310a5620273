"""uwie_diff_gated_u8 / Device.diff_gated_u8 / GatedDifferentiableEnhancement.enhance_u8 on the device.

The oracle is the float32 route, which this entry point shares no kernel launch with: u8_to_f32, the digit-pass selection
over the float image and k_diff_gated (itself pinned to the reference's goldens).  Both end in the same per-value source
(devutil.h gated_px), so the float outputs are compared word for word and the bytes exactly.  The CPU restatement
(tests/gated_u8_ref.py, pinned by tests/test_gated_u8_ref.py) is compared bit for bit where use_gamma = 0 and within 2^-23
elsewhere, the gated forward's tolerance against torch on the CPU (tests/test_gpu_dlp_grad.py): the two
pow differ by at most one ulp of z <= 1, 2^-24, which use_gamma <= 1 scales; the product and the sum round once more on
each side (2^-25 each at most below 1)."""
import numpy as np
import pytest

import gated_u8_cases as C
import gated_u8_ref as R

pytestmark = pytest.mark.gpu

STATUS_DIFF_RANK = 16


@pytest.fixture(scope="module")
def dev():
    import underwater_image_enhancement_amd as uw

    return uw.get_device(0)


def up(dev, a):
    """a (read-only) case array on the device"""
    return dev.tensor(np.array(a))


def bits(t):
    """a float32 device tensor as its int32 words on the host"""
    import torch

    return t.contiguous().view(torch.int32).cpu().numpy()


def float_route(dev, u8, cols):
    """(float32 [B,H,W,3], its clipped * 255 truncation) by the float32 route; no image of these cases is flagged"""
    import torch

    f = dev.diff_gated_f32(dev.u8_to_f32(u8), cols, planar=False)
    return f, (f.clamp(0.0, 1.0) * 255).to(torch.uint8)


def check_equivalence(dev, name, u8, cols):
    want_f, want_q = float_route(dev, u8, cols)
    got_q, got_f = dev.diff_gated_u8(u8, cols, want_u8=True, want_f32=True)
    assert got_q.dtype == want_q.dtype and tuple(got_q.shape) == tuple(u8.shape) == tuple(got_f.shape)
    nf = int(np.count_nonzero(bits(got_f) != bits(want_f)))
    nq = int(np.count_nonzero(got_q.cpu().numpy() != want_q.cpu().numpy()))
    print(f"{name}: {nf} float words differ, {nq} bytes differ")
    assert nf == 0 and nq == 0, name
    # each output alone gives the same
    only_q, none = dev.diff_gated_u8(u8, cols, want_u8=True, want_f32=False)
    assert none is None and np.array_equal(only_q.cpu().numpy(), got_q.cpu().numpy())
    none, only_f = dev.diff_gated_u8(u8, cols, want_u8=False, want_f32=True)
    assert none is None and np.array_equal(bits(only_f), bits(got_f))
    assert dev.check_status() == 0
    return got_q, got_f


@pytest.mark.parametrize("name", C.names())
def test_equals_the_float32_route(dev, name):
    c = C.case(name)
    got_q, got_f = check_equivalence(dev, name, up(dev, c["u8"]), up(dev, c["cols"]))
    # and the CPU restatement
    want = R.float_image(c["u8"], c["cols"])
    got = got_f.cpu().numpy()
    assert np.all(got >= 0.0) and np.all(got <= 1.0)
    for b in range(got.shape[0]):
        if c["cols"][b, 2] == 0:
            assert R.same_bits(got[b], want[b]) and np.array_equal(got_q[b].cpu().numpy(), R.quantise(want[b])), (name, b)
        else:
            d = np.abs(got[b].astype(np.float64) - want[b].astype(np.float64)).max()
            print(f"{name} image {b}: {d:.3g} from torch's CPU operations")
            assert d <= 2.0 ** -23, (name, b, d)


def test_gamma_nan(dev):
    name, u8, cols = C.NAN_GAMMA
    _, got_f = check_equivalence(dev, name, up(dev, u8), up(dev, cols))
    assert not np.isnan(got_f.cpu().numpy()).any()  # the final clamp leaves no NaN behind: the image is not flagged


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("L,exc", C.UNINDEXABLE)
def test_unindexable_position(dev, L, exc, which):
    import underwater_image_enhancement_amd as uw

    rng = np.random.default_rng(5)
    u8 = np.stack([C.step_frame(40), rng.integers(0, 256, (10, 10, 3), dtype=np.uint8), C.step_frame(70)])
    cols = np.array([[10.0, 90.0, 0.5, 1.2], [20.0, 80.0, 0.7, 1.4], [-3.6, 95.0, 1.0, 0.8]], np.float32)
    good = cols.copy()
    cols[1, which] = L
    d8, dc = up(dev, u8), up(dev, cols)
    assert dev.check_status() == 0
    got_q, got_f, saved = dev.diff_gated_u8(d8, dc, want_u8=True, want_f32=True, saved=True)
    assert dev.check_status(allow=STATUS_DIFF_RANK) == STATUS_DIFF_RANK
    assert dev.check_status() == 0  # cleared
    f, q = got_f.cpu().numpy(), got_q.cpu().numpy()
    assert np.isnan(f[1]).all() and not q[1].any()
    # the other images are what they are alone, and what the float32 route gives them
    for b in (0, 2):
        one_q, one_f = dev.diff_gated_u8(d8[b:b + 1], up(dev, good[b:b + 1]), want_u8=True, want_f32=True)
        assert np.array_equal(bits(one_f)[0], f[b].view(np.int32)) and np.array_equal(one_q.cpu().numpy()[0], q[b]), b
    want_f, want_saved = dev.diff_gated_save_f32(dev.u8_to_f32(d8), dc, planar=False)
    assert dev.check_status(allow=STATUS_DIFF_RANK) == STATUS_DIFF_RANK
    assert np.array_equal(bits(want_f), f.view(np.int32)) and np.array_equal(bits(want_saved), bits(saved))
    # Python raises what GatedDifferentiableEnhancement raises
    mod = uw.GatedDifferentiableEnhancement()
    par = {k: cols[:, i:i + 1] for i, k in enumerate(mod.KEYS)}
    with pytest.raises(exc):
        mod(u8.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0), par)
    for out in ("u8", "float32"):
        with pytest.raises(exc):
            mod.enhance_u8(u8, par, out=out)
    assert dev.check_status() == 0


def test_bytes_do_not_depend_on_the_batch(dev):
    c = C.case("shape_5x33x95")
    whole, _ = dev.diff_gated_u8(up(dev, c["u8"]), up(dev, c["cols"]))
    whole = whole.cpu().numpy()
    for b in range(5):
        one, _ = dev.diff_gated_u8(up(dev, c["u8"][b:b + 1]), up(dev, c["cols"][b:b + 1]))
        assert np.array_equal(one.cpu().numpy()[0], whole[b]), b
    order = [3, 0, 4, 2, 1, 3, 3]
    perm, _ = dev.diff_gated_u8(up(dev, c["u8"][order]), up(dev, c["cols"][order]))
    assert np.array_equal(perm.cpu().numpy(), whole[order])


def test_two_runs_give_the_same_bits(dev):
    c = C.case("shape_2x257x511")
    u8, cols = up(dev, c["u8"]), up(dev, c["cols"])
    a = dev.diff_gated_u8(u8, cols, want_u8=True, want_f32=True)
    b = dev.diff_gated_u8(u8, cols, want_u8=True, want_f32=True)
    assert np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy()) and np.array_equal(bits(a[1]), bits(b[1]))


@pytest.mark.parametrize("name", ["shape_3x5x3", "shape_5x33x95", "rank_k_eq_rank", "rank_k_eq_rank_plus_1", "rank_negative",
                                  "rank_low_above_high", "rank_low_eq_high"])
def test_saved_equals_the_float32_forward(dev, name):
    c = C.case(name)
    u8, cols = up(dev, c["u8"]), up(dev, c["cols"])
    _, want = dev.diff_gated_save_f32(dev.u8_to_f32(u8), cols, planar=False)
    q, f, saved = dev.diff_gated_u8(u8, cols, want_u8=True, want_f32=False, saved=True)
    assert f is None and tuple(saved.shape) == (c["u8"].shape[0], 3, 2)
    assert np.array_equal(bits(saved), bits(want))
    assert np.array_equal(saved.cpu().numpy(), R.order_statistics(c["u8"], c["cols"]))


def test_module_enhance_u8(dev):
    import underwater_image_enhancement_amd as uw

    c = C.case("shape_5x33x95")
    mod = uw.GatedDifferentiableEnhancement()
    par = {k: c["cols"][:, i:i + 1] for i, k in enumerate(mod.KEYS)}
    want_f, want_q = float_route(dev, up(dev, c["u8"]), up(dev, c["cols"]))
    got = mod.enhance_u8(c["u8"], par)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want_q.cpu().numpy())
    on_dev = mod.enhance_u8(up(dev, c["u8"]), par, out="float32")
    assert on_dev.is_cuda and np.array_equal(bits(on_dev), bits(want_f))
    # forward's own bits for u8 / 255, in its (B, 3, H, W) layout
    fwd = mod(dev.u8_to_f32(up(dev, c["u8"])).permute(0, 3, 1, 2).contiguous(), par)
    assert np.array_equal(bits(fwd.permute(0, 2, 3, 1)), bits(on_dev))
    one = mod.enhance_u8(c["u8"][2], {k: v[2:3] for k, v in par.items()})
    assert one.shape == (33, 95, 3) and np.array_equal(one, got[2])
    with pytest.raises(TypeError):
        mod.enhance_u8(c["u8"].astype(np.float32), par)
    with pytest.raises(ValueError):
        mod.enhance_u8(c["u8"], par, out="f16")
    with pytest.raises(KeyError):
        mod.enhance_u8(c["u8"], {k: v for k, v in par.items() if k != "gamma"})
