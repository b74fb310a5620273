"""What the cases of tests/fusion_cases.py are for, proven on the NumPy statement of the contract (tests/fusion_ref.py) alone: no
device.  tests/test_gpu_fusion.py then holds the kernels to the same reference on the same cases."""
import numpy as np
import pytest

import fusion_cases as K
import fusion_ref as ref


@pytest.mark.parametrize("levels", range(1, 9))
def test_flat_frame_is_the_mean_of_the_two_inputs(levels):
    """A frame of one level v: I1 = G[v], I2 = v, both weights equal, Wn = 0.5 exactly, out = rint((G[v] + v) / 2)."""
    for gamma in (2.2, 0.8):
        G = ref.table(gamma)
        for v in (0, 1, 77, 128, 200, 255):
            out, in1, in2, wn = ref.fusion(np.full((5, 6, 3), v, np.uint8), gamma, levels)
            assert (in1 == G[v]).all() and (in2 == v).all() and (wn == 0.5).all()
            assert (out == np.rint((float(G[v]) + v) / 2)).all(), (gamma, v, levels)
    # the tie: G[77] = 18 at gamma 2.2, (18 + 77) / 2 = 47.5 -> 48 (half to even)
    assert ref.table(2.2)[77] == 18
    assert (K.reference(K.case("flat_77"), 2.2, levels)[0] == 48).all()


def test_reduce_and_expand_keep_a_constant_plane():
    for value in (0.5, 0.1, 1.0 / 3.0, 254.7, -17.25, 1e-300):
        for h, w in ((1, 1), (1, 5), (5, 1), (2, 3), (7, 4), (9, 9)):
            for dtype in (np.float64, np.float32):
                p = np.full((h, w), value, dtype)
                r = ref.reduce(p)
                assert r.shape == ((h + 1) // 2, (w + 1) // 2) and (r == p[0, 0]).all(), (value, h, w)
                e = ref.expand(r, h, w)
                assert e.shape == (h, w) and (e == p[0, 0]).all(), (value, h, w)


def test_one_level_is_the_per_pixel_blend():
    for c in (K.case("scene_33x47"), K.case("clipping")):
        out, in1, in2, wn = K.reference(c, 2.2, 1)
        v = in2.astype(np.float64) + wn[..., None] * (in1.astype(np.int64) - in2.astype(np.int64)).astype(np.float64)
        assert np.array_equal(out, np.rint(np.clip(v, 0, 255)).astype(np.uint8))


@pytest.mark.parametrize("name,op", [("flip_ud", lambda a: a[::-1]), ("flip_lr", lambda a: a[:, ::-1]),
                                     ("transpose", lambda a: np.swapaxes(a, 0, 1))])
def test_one_level_is_equivariant(name, op):
    """Every term of the weight and both inputs are symmetric under the flips and the transpose (the binomial blur is a sum of
    symmetric integer taps; the Laplacian subtracts four integers), so at L = 1 the result moves with the frame bit for bit."""
    c = K.case("scene_33x47")
    want = K.reference(c, 2.2, 1)
    got = ref.fusion(np.ascontiguousarray(op(c.frame)), 2.2, 1)
    for g, w in zip(got, want):
        assert np.array_equal(g, op(w)), name
    assert np.array_equal(got[3].view(np.uint64), np.ascontiguousarray(op(want[3])).view(np.uint64))


@pytest.mark.parametrize("gamma", K.TABLE_GAMMAS)
def test_table_entries_are_far_from_a_half(gamma):
    """No entry of 255 (v / 255)^gamma lies within 2e-4 of a half: an ulp of pow() cannot move the byte."""
    v = np.arange(256, dtype=np.float64)
    t = 255.0 * (v / 255.0) ** gamma
    assert np.abs(t - np.floor(t) - 0.5).min() >= 2e-4
    assert np.array_equal(ref.table(gamma), np.rint(t).astype(np.uint8))
    assert ref.table(gamma)[0] == 0 and ref.table(gamma)[255] == 255


def test_gamma_one_is_the_identity_table():
    assert np.array_equal(ref.table(1.0), np.arange(256, dtype=np.uint8))


def test_float32_changes_a_byte():
    c = K.case("f32_sensitive")
    out = K.reference(c, *K.F32_PARAMS)[0]
    f32 = ref.fusion(c.frame, *K.F32_PARAMS, dtype=np.float32)[0]
    assert 1 <= np.count_nonzero(out != f32) <= 8
    assert np.abs(out.astype(int) - f32.astype(int)).max() == 1


def test_clipping_frame_clips_at_both_ends():
    c = K.case("clipping")
    x = c.frame.astype(np.int64)
    raw = (512 * x - ref.blur(x) + 128) >> 8
    assert (raw < 0).any() and (raw > 255).any()  # the clamp of I2 works at both ends
    _, _, in2, wn = K.reference(c, 0.8, 1)
    acc = ref.fuse(ref.table(0.8)[c.frame], in2, wn, 4)
    v = in2 + acc
    assert (v <= 0).any() and (v >= 255).any()
    out = K.reference(c, 0.8, 4)[0]
    assert (out == 0).any() and (out == 255).any()


def test_tiny_and_parity_shapes_are_valid_at_every_level_count():
    for h, w in K.TINY_SHAPES:
        c = K.case(f"scene_{h}x{w}")
        for levels in (1, 2, 8):
            out, in1, in2, wn = K.reference(c, 1.5, levels)
            assert out.shape == (h, w, 3) and wn.shape == (h, w) and np.isfinite(wn).all() and ((wn > 0) & (wn < 1)).all()
    sizes = lambda h, w, n: [((h + (1 << l) - 1) >> l, (w + (1 << l) - 1) >> l) for l in range(n)]  # noqa: E731
    assert sizes(37, 21, 6)[-2:] == [(3, 2), (2, 1)] and sizes(37, 21, 8)[-2:] == [(1, 1), (1, 1)]
    assert {h % 2 for h, _ in sizes(33, 47, 6)} == {0, 1} and {w % 2 for _, w in sizes(33, 47, 6)} == {0, 1}
    assert ref.fusion(K.case("scene_37x21").frame, 2.2, 6)[0].shape == (37, 21, 3)


def test_shapes_straddle_the_plan():
    tw, th = K.plan()
    shapes = {c.shape for c in K.all_cases()}
    for w in (tw - 1, tw, tw + 1, 2 * tw + 3):
        assert any(s[1] == w for s in shapes), w
    for h in (th - 1, th, th + 1, 2 * th + 3):
        assert any(s[0] == h for s in shapes), h
    (H, W), pos = K.impulse_positions(tw, th)
    for d in range(6):
        assert any(y == d for y, _ in pos) and any(x == d for _, x in pos)
        assert any(y == H - 1 - d for y, _ in pos) and any(x == W - 1 - d for _, x in pos)
    for k in (1, 2):
        for side in (-1, 0):
            assert any(y == k * th + side for y, _ in pos) and any(x == k * tw + side for _, x in pos)


def test_an_impulse_reaches_across_a_seam():
    """The raised pixel changes I1 at its own place only and I2 out to distance 2, on both sides of the tile seam it sits on; the
    frame's means move with it, so Wn changes everywhere."""
    tw, th = K.plan()
    c = K.case(f"impulse_{th}_{tw}")
    ground = ref.fusion(np.zeros_like(c.frame) + c.frame[0, 0], 2.2, 3)
    got = K.reference(c, 2.2, 3)
    ys, xs = np.nonzero((got[1] != ground[1]).any(-1))
    assert (ys.tolist(), xs.tolist()) == ([th], [tw])
    ys, xs = np.nonzero((got[2] != ground[2]).any(-1))
    assert ys.min() == th - 2 and ys.max() == th + 2 and xs.min() == tw - 2 and xs.max() == tw + 2
    assert (got[3] != ground[3]).all()


def test_default_levels():
    assert [ref.default_levels(m, 4000) for m in (1, 7, 8, 15, 16, 32, 270, 1080, 2160)] == [1, 1, 1, 1, 2, 3, 6, 6, 6]
