"""uwie_diff_enhance_u8 / Device.diff_enhance_u8 and the predictor's byte route on the device.

The main oracle is the float32 route, which this entry point shares no kernel launch with: u8_to_f32, the digit-pass
selection over the float image and k_diff_enhance (itself pinned to the reference's goldens).  Both end in the same per-pixel
source (devutil.h vgg_after_stretch, pow_f32_fast), so the float outputs are compared bit for bit and the bytes exactly.
The CPU oracle (tests/diffenh_u8_ref.py, equal to oracle.diff_enhance: tests/test_diffenh_u8_ref.py) is compared bit for bit
where there is no pow, and at the module's <= 1 float32 ulp where there is."""
import os

import numpy as np
import pytest

import diffenh_u8_cases as C
import diffenh_u8_ref as R
import param_net_ref as PN

pytestmark = pytest.mark.gpu

PRED_SIZE = 48


@pytest.fixture(scope="module")
def dev():
    import underwater_image_enhancement_amd as uw

    return uw.get_device(0)


@pytest.fixture(scope="module")
def predictor():
    import underwater_image_enhancement_amd as uw

    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "param_net.npz"), allow_pickle=False) as z:
        seed = int(z["seed"])
    return uw.EnhancementPredictor(PN.seeded_state(seed), input_size=PRED_SIZE)


def up(dev, a):
    """a (read-only) case array on the device"""
    return dev.tensor(np.array(a))


def bits(t):
    """a float32 device tensor as its int32 words on the host"""
    import torch

    return t.contiguous().view(torch.int32).cpu().numpy()


def parent_route(dev, u8, cols, flags):
    """(float32 [B,H,W,3], its bytes) by the float32 route and the predictor's torch passes"""
    import torch

    f = dev.diff_enhance_f32(dev.u8_to_f32(u8), cols, planar=False, has_omega=bool(flags & 1), has_gamma=bool(flags & 2))
    q = (f.clone().clamp_(0.0, 1.0).nan_to_num_(nan=0.0, posinf=1.0, neginf=0.0).clamp_(0.0, 1.0) * 255).to(torch.uint8)
    return f, q


@pytest.mark.parametrize("name", C.names())
def test_equals_the_float32_route(dev, name):
    c = C.case(name)
    u8, cols = up(dev, c["u8"]), up(dev, c["cols"])
    for flags in (0, 1, 2, 3):
        want_f, want_q = parent_route(dev, u8, cols, flags)
        got_q, got_f = dev.diff_enhance_u8(u8, cols, flags, want_u8=True, want_f32=True)
        assert got_q.dtype == want_q.dtype and tuple(got_q.shape) == tuple(u8.shape)
        nf = int(np.count_nonzero(bits(got_f) != bits(want_f)))
        nq = int(np.count_nonzero(got_q.cpu().numpy() != want_q.cpu().numpy()))
        print(f"{name} flags {flags}: {nf} float words differ, {nq} bytes differ")
        assert nf == 0 and nq == 0, (name, flags)
        # each output alone gives the same
        only_q, none = dev.diff_enhance_u8(u8, cols, flags, want_u8=True, want_f32=False)
        assert none is None and np.array_equal(only_q.cpu().numpy(), got_q.cpu().numpy())
        none, only_f = dev.diff_enhance_u8(u8, cols, flags, want_u8=False, want_f32=True)
        assert none is None and np.array_equal(bits(only_f), bits(got_f))
    dev.check_status()


@pytest.mark.parametrize("name", C.names(finite_only=True))
def test_against_the_cpu_oracle(dev, name):
    c = C.case(name)
    u8, cols = up(dev, c["u8"]), up(dev, c["cols"])
    for flags in ((0, 1, 2, 3) if c["u8"].size < 10 ** 6 else (1, 3)):
        want = R.float_image(c["u8"], c["cols"], flags)
        got_q, got_f = dev.diff_enhance_u8(u8, cols, flags, want_u8=True, want_f32=True)
        got = got_f.cpu().numpy()
        if not flags & 2:
            assert R.same_bits(got, want), (name, flags)
            assert np.array_equal(got_q.cpu().numpy(), R.quantise(want)), (name, flags)
        else:  # pow: <= 1 float32 ulp (values in [0, 1]: the int32 words are ordered as the values)
            assert np.all(got >= 0.0) and np.all(got <= 1.0)
            ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()
            print(f"{name} flags {flags}: {ulp} ulp")
            assert ulp <= 1, (name, flags)


def test_bytes_do_not_depend_on_the_batch(dev):
    c = C.case("shape_5x33x95")
    whole, _ = dev.diff_enhance_u8(up(dev, c["u8"]), up(dev, c["cols"]))
    whole = whole.cpu().numpy()
    for b in range(5):
        one, _ = dev.diff_enhance_u8(up(dev, c["u8"][b:b + 1]), up(dev, c["cols"][b:b + 1]))
        assert np.array_equal(one.cpu().numpy()[0], whole[b]), b
    order = [3, 0, 4, 2, 1, 3, 3]
    perm, _ = dev.diff_enhance_u8(up(dev, c["u8"][order]), up(dev, c["cols"][order]))
    assert np.array_equal(perm.cpu().numpy(), whole[order])


def test_two_runs_give_the_same_bits(dev):
    c = C.case("shape_2x257x511")
    u8, cols = up(dev, c["u8"]), up(dev, c["cols"])
    a = dev.diff_enhance_u8(u8, cols, 3, want_u8=True, want_f32=True)
    b = dev.diff_enhance_u8(u8, cols, 3, want_u8=True, want_f32=True)
    assert np.array_equal(a[0].cpu().numpy(), b[0].cpu().numpy()) and np.array_equal(bits(a[1]), bits(b[1]))


@pytest.mark.parametrize("name", ["shape_3x5x3", "shape_5x33x95", "rank_k_eq_rank", "rank_k_eq_rank_plus_1", "rank_low_above_high"])
def test_saved_equals_the_float32_forward(dev, name):
    c = C.case(name)
    u8, cols = up(dev, c["u8"]), up(dev, c["cols"])
    _, want = dev.diff_enhance_save_f32(dev.u8_to_f32(u8), cols, planar=False, flags=3)
    q, f, saved = dev.diff_enhance_u8(u8, cols, 3, want_u8=True, want_f32=False, saved=True)
    assert f is None and tuple(saved.shape) == (c["u8"].shape[0], 3, 2)
    assert np.array_equal(bits(saved), bits(want))
    assert np.array_equal(saved.cpu().numpy(), R.order_statistics(c["u8"], c["cols"]))


def test_module_enhance_u8(dev):
    import underwater_image_enhancement_amd as uw

    c = C.case("shape_5x33x95")
    mod = uw.DifferentiableEnhancement()
    par = {"L_low": c["cols"][:, 0:1], "L_high": c["cols"][:, 1:2], "omega": c["cols"][:, 2:3], "gamma": c["cols"][:, 3:4]}
    want_f, want_q = parent_route(dev, up(dev, c["u8"]), up(dev, c["cols"]), 3)
    got = mod.enhance_u8(c["u8"], par)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want_q.cpu().numpy())
    on_dev = mod.enhance_u8(up(dev, c["u8"]), par, out="float32")
    assert on_dev.is_cuda and np.array_equal(bits(on_dev), bits(want_f))
    one = mod.enhance_u8(c["u8"][2], {k: v[2:3] for k, v in par.items()})
    assert one.shape == (33, 95, 3) and np.array_equal(one, got[2])
    # a missing key skips its stage, as in forward
    no_gamma = mod.enhance_u8(c["u8"], {k: v for k, v in par.items() if k != "gamma"}, out="float32")
    assert np.array_equal(no_gamma.view(np.int32), bits(parent_route(dev, up(dev, c["u8"]), up(dev, c["cols"]), 1)[0]))
    with pytest.raises(TypeError):
        mod.enhance_u8(c["u8"].astype(np.float32), par)
    with pytest.raises(ValueError):
        mod.enhance_u8(c["u8"], par, out="f16")
    with pytest.raises(KeyError):
        mod.enhance_u8(c["u8"], {"omega": par["omega"]})


def test_predictor_enhance_batch_u8(dev, predictor):
    import torch

    rng = np.random.default_rng(21)
    frames = rng.integers(0, 256, (3, 40, 56, 3), dtype=np.uint8)
    out, params = predictor.enhance_batch_u8(frames)
    assert out.is_cuda and out.dtype == torch.uint8 and tuple(out.shape) == (3, 40, 56, 3)
    assert params.is_cuda and params.dtype == torch.float32 and tuple(params.shape) == (3, 4)
    want = (predictor.enhance_batch(frames) * 255).to(torch.uint8)
    assert np.array_equal(out.cpu().numpy(), want.cpu().numpy())
    assert np.array_equal(bits(params), bits(predictor._clamped(dev, dev.tensor(frames))))
    # the float forms of the same frames
    for x in (dev.tensor(frames), frames.astype(np.float32) / np.float32(255.0), frames / 255):
        again, p = predictor.enhance_batch_u8(x)
        assert np.array_equal(again.cpu().numpy(), out.cpu().numpy()) and np.array_equal(bits(p), bits(params))


def test_predictor_process_frames(dev, predictor):
    rng = np.random.default_rng(22)
    sizes = [(40, 56), (24, 32), (40, 56), (17, 9), (24, 32), (40, 56)]
    frames = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    frames.insert(3, rng.integers(0, 256, (24, 32, 3)).astype(np.int32))  # a frame the predictor does not take
    frames[5] = frames[5] / 255                                           # a float image u8 / 255
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
