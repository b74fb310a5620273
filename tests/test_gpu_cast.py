"""Cast detection (detect_image_type, six_stadigy.py:292-302) on the device against NumPy, at every path of the closed-form
restatement of NumPy's sequential float32 mean (k_entry.hip: k_chunk_hist, k_chunk_hist_quad, k_chunk_ulps, k_cast_resolve,
k_cast_decide) and of the general-float route (k_float.hip: k_f_mean_seq).  The frames and what they reach are in
tests/cast_cases.py; tests/test_cast_cases.py asserts on the CPU that they reach it.

Everything is exact equality: the means float for float with ``img.mean(axis=(0, 1))``, the kind with the oracle's, the bits
the same whatever batch a frame sits in and however often the call is repeated.
"""
import numpy as np
import pytest

import cast_cases as cc

pytestmark = pytest.mark.gpu

KINDS = ["normal", "greenish", "bluish"]
_WANT = {}


@pytest.fixture(scope="module")
def dev():
    import underwater_image_enhancement_amd as uw

    return uw.get_device(0)


@pytest.fixture(scope="module")
def orc():
    from oracle import uwie_oracle

    return uwie_oracle


def want(orc, name):
    """(float32 [3], kind index): NumPy's own mean of the normalised frame and the oracle's decision, computed once."""
    if name not in _WANT:
        x = orc.normalise_u8(cc.case(name).u8)
        _WANT[name] = (x.mean(axis=(0, 1)), KINDS.index(orc.classify_cast(x)))
        if name in cc.KINDS:
            assert KINDS[_WANT[name][1]] == cc.KINDS[name]
    return _WANT[name]


def same(got, want_, what):
    got, want_ = np.asarray(got), np.asarray(want_)
    assert got.dtype == want_.dtype and got.shape == want_.shape, (what, got.dtype, want_.dtype, got.shape, want_.shape)
    if got.tobytes() != want_.tobytes():
        bits = (lambda a: [hex(v) for v in a.ravel().view(np.uint32)]) if got.dtype.itemsize == 4 else (lambda a: a.tolist())
        raise AssertionError(f"{what}: got {got.tolist()} {bits(got)} want {want_.tolist()} {bits(want_)}")


def classify(dev, batch):
    kind, mean = dev.cast_classify(dev.tensor(batch))
    dev.check_status()
    return kind.cpu().numpy(), mean.cpu().numpy()


# ------------------------------------------------------------------ uwie_cast_classify
@pytest.mark.parametrize("name", cc.NAMES)
def test_single_frame(dev, orc, name):
    u8 = cc.case(name).u8
    mean_w, kind_w = want(orc, name)
    kind, mean = classify(dev, u8[None])
    same(mean[0], mean_w, name)
    assert int(kind[0]) == kind_w, name
    kind2, mean2 = classify(dev, u8[None])  # the same bits again
    same(mean2, mean, name)
    same(kind2, kind, name)


def batch_groups():
    """The frames that share a shape, by construction: the 64 x 64 frames of case 9, the pairs of case 10, the five frames of
    case 11; every other frame is alone with its filler."""
    together = {9: [], 10: [], 11: []}
    groups = []
    for name in cc.NAMES:
        if cc.GROUP[name] in together:
            if not together[cc.GROUP[name]]:
                groups.append(together[cc.GROUP[name]])
            together[cc.GROUP[name]].append(name)
        else:
            groups.append([name])
    return groups


@pytest.mark.parametrize("group", batch_groups(), ids=lambda g: g[0] + (f"+{len(g) - 1}" if len(g) > 1 else ""))
def test_inside_batches(dev, orc, group):
    """The frames of one shape in two compositions: behind a filler frame (the last of them is the batch's last frame, where
    the drill may not read past its pixels), and in reverse order -- a lone frame in front of the filler, so that it is not the
    last.  Case 11's five frames of 7 chunks are 35 chunks in the second composition: three k_chunk_ulps blocks of 16 with the
    frame borders inside them.  A frame's result is the single-frame result bit for bit wherever it sits."""
    frames = [cc.case(n).u8 for n in group]
    filler = np.ascontiguousarray(np.roll(frames[0], 1, axis=2))  # the first frame with its channels rotated
    filler_mean = np.roll(want(orc, group[0])[0], 1)
    first = [None] + group
    second = group[::-1] if len(group) > 1 else [group[0], None]
    for names in (first, second):
        batch = np.stack([filler if n is None else cc.case(n).u8 for n in names])
        kind, mean = classify(dev, batch)
        for i, n in enumerate(names):
            if n is None:
                same(mean[i], filler_mean, (names, i))
            else:
                mean_w, kind_w = want(orc, n)
                same(mean[i], mean_w, (names, i))
                assert int(kind[i]) == kind_w, (names, i)
        kind2, mean2 = classify(dev, batch)
        same(mean2, mean, names)
        same(kind2, kind, names)


# ------------------------------------------------------------------ uwie_cast_classify_f32 (k_f_mean_seq)
def classify_f32(dev, batch):
    kind, mean = dev.cast_classify_f32(dev.tensor(batch))
    dev.check_status()
    return kind.cpu().numpy(), mean.cpu().numpy()


@pytest.mark.parametrize("name", cc.NAMES)
def test_general_float_route_on_the_same_streams(dev, orc, name):
    x = orc.normalise_u8(cc.case(name).u8)
    mean_w, kind_w = want(orc, name)
    kind, mean = classify_f32(dev, x[None])
    same(mean[0], mean_w, name)
    assert int(kind[0]) == kind_w, name


def test_general_float_route_on_a_batch(dev, orc):
    names = [n for n in cc.NAMES if cc.GROUP[n] == 11]
    kind, mean = classify_f32(dev, np.stack([orc.normalise_u8(cc.case(n).u8) for n in names]))
    for i, n in enumerate(names):
        same(mean[i], want(orc, n)[0], n)
        assert int(kind[i]) == want(orc, n)[1], n


def test_general_float_images(dev, orc):
    for name, x in cc.general_float_images().items():
        kind, mean = classify_f32(dev, x[None])
        same(mean[0], x.mean(axis=(0, 1)), name)
        assert KINDS[int(kind[0])] == orc.classify_cast(x), name


# ------------------------------------------------------------------ the fused chunk pass (k_chunk_hist_quad) through the pipeline
FUSED = [n for n in cc.NAMES if cc.GROUP[n] in (10, 12)]


def _other_kind(name, kind):
    if cc.GROUP[name] == 10:  # the decision the frame's twin gets
        cast = KINDS.index(name.split("_")[1])
        return cast if kind == 0 else 0
    return (kind + 1) % 3


@pytest.mark.parametrize("name", FUSED)
def test_fused_chunk_pass_decides_like_the_oracle(dev, orc, name):
    """k_chunk_hist_quad's means cannot be read, its decision can: enhance_all_u8 returns the pipeline's own kinds, and the
    bytes of enhance_u8 are those of the run with the oracle's kind forced and not those with the other kind forced.  The
    pairs of case 10 are one level of one pixel apart and fall on either side: one miscounted pixel decides wrongly."""
    from underwater_image_enhancement_amd import _lib

    u8 = cc.case(name).u8
    kind_w = want(orc, name)[1]
    frames = dev.tensor(u8[None])
    p = dev.params(_lib.SURFACE_SIX, 2)
    got = {}
    for fuse in (0, 1, 2):
        with dev.tuning(entry_fuse=fuse):
            out, _ = dev.enhance_u8(frames, p)
            dev.check_status()
            _, kinds = dev.enhance_all_u8(frames)
            dev.check_status()
        assert kinds.cpu().numpy().tolist() == [kind_w], (name, fuse)
        got[fuse] = out.cpu().numpy()
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2]), name
    forced, _ = dev.enhance_u8(frames, dev.params(_lib.SURFACE_SIX, 2, forced_cast=kind_w))
    dev.check_status()
    assert np.array_equal(forced.cpu().numpy(), got[1]), name
    wrong, _ = dev.enhance_u8(frames, dev.params(_lib.SURFACE_SIX, 2, forced_cast=_other_kind(name, kind_w)))
    dev.check_status()
    assert not np.array_equal(wrong.cpu().numpy(), got[1]), name


@pytest.mark.parametrize("kind", ["greenish", "bluish"])
def test_fused_chunk_pass_on_a_pair_in_one_batch(dev, orc, kind):
    names = [f"pair_{kind}_normal", f"pair_{kind}_cast", f"pair_{kind}_normal"]
    frames = dev.tensor(np.stack([cc.case(n).u8 for n in names]))
    for fuse in (0, 1, 2):
        with dev.tuning(entry_fuse=fuse):
            _, kinds = dev.enhance_all_u8(frames)
            dev.check_status()
        assert kinds.cpu().numpy().tolist() == [want(orc, n)[1] for n in names], (kind, fuse)


@pytest.mark.parametrize("name", [n for n in cc.NAMES if cc.GROUP[n] == 12])
def test_quadrant_histograms_of_the_fused_pass_on_its_shapes(dev, orc, name):
    """The level-0 quadrant histograms the chunk pass leaves for the quadtree, on the shapes of case 12: the atmospheric light
    with and without trace is the same for every entry_fuse setting, and the oracle's."""
    u8 = cc.case(name).u8
    kind_w = want(orc, name)[1]
    frames = dev.tensor(u8[None])
    kk = dev.tensor(np.array([kind_w], np.int32))
    got = {}
    for fuse in (0, 1, 2):
        with dev.tuning(entry_fuse=fuse):
            A, tr = dev.atmospheric_light(frames, kk, trace=True)
            A2 = dev.atmospheric_light(frames, kk)
            dev.check_status()
        got[fuse] = (A.cpu().numpy(), tr.tobytes(), A2.cpu().numpy())
    xc = orc.correct_cast(orc.normalise_u8(u8), KINDS[kind_w])
    want_A = np.asarray(orc.atmospheric_light(xc, 1))
    for fuse in (0, 1, 2):
        same(got[fuse][0][0], want_A, (name, fuse))
        same(got[fuse][2][0], want_A, (name, fuse))
        assert got[fuse][1] == got[0][1], (name, fuse)
