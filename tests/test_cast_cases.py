"""CPU preconditions of tests/test_gpu_cast.py: every frame of tests/cast_cases.py is what it claims to be, by the analyser
(NumPy's own float32 accumulation) and the oracle alone.  Nothing here touches the device, so a defect of the kernels cannot
make a precondition pass or fail; and tests/test_gpu_cast.py cannot pass vacuously, because the paths it is aimed at are
asserted to be reached here.

The cases (numbers are Case.group):
   1 walk lanes         crossing-drilled chunks at walk lanes 0, 1, 63 and behind 64 clean chunks; 1, 63, 64, 65 chunks left
   2 drill positions    crossings at threads 0, 63, 64, 1023 and pixels 0, 15 without a head; thread 64 behind a head; two in one thread
   3 several binades    chunks with exactly 2 and with >= 3 crossings; gains 0, 1, >= 2 in front of a walked chunk
   4 exact landings     all-255 content: the sum hits every power of two; 128 x 128 lands on its last pixel; shifted landings
   5 ties               >= 16 ties outside any head, >= 4 either way, >= 3 chunks, a chunk drilled for a tie alone
   6 tiny accumulator   chunks that stay below 0.25, then past it in the middle of a chunk
   7 frame tails        npx % 16384 in {0, 1, 15, 16, 17}, the last chunk drilled
   8 saturation         2^24 + 12288 pixels of 255 / 254 / both: the mean is 2^24 / npx on all three channels
   9 threshold          g - r (b - r) one ulp below, at, one ulp above float32(0.05); g == b; g == r
  10 threshold pairs    264 x 512 frames one level of one pixel apart on either side of the decision
  11 seven chunks       five different frames of 7 chunks: 35 chunks are three k_chunk_ulps blocks with frame borders inside
  12 fused shapes       (6, 16384), (1030, 64), (333, 264) for k_chunk_hist_quad
"""
import numpy as np
import pytest

import cast_cases as cc

F32 = np.float32


def reports(name):
    return [cc.report(name, c) for c in range(3)]


def by_group(g):
    return [n for n in cc.NAMES if cc.GROUP[n] == g]


@pytest.mark.parametrize("name", cc.NAMES)
def test_numpy_reduces_sequentially_and_the_analyser_agrees(name):
    """img.mean(axis=(0, 1)) is the sequential float32 sum per channel, divided in float64.  If the installed NumPy reduces in
    another order this fails first: every other file of this suite is then aimed at the wrong value."""
    u8 = cc.case(name).u8
    x = u8.astype(F32) / F32(255)
    got = x.mean(axis=(0, 1))
    want = cc.sequential_mean(name)
    assert got.dtype == F32 and np.array_equal(got, want), f"NumPy's mean is not the sequential float32 sum: {got!r} vs {want!r}"
    assert u8.nbytes <= 8 << 20 or name == "saturation"  # sparse streams, not large dense frames
    for c in range(3):  # zeros in front change nothing: what the sparse streams rely on
        if name != "saturation":
            r = cc.report(name, c)
            shifted = np.concatenate([np.zeros(1000, F32), x[:, :, c].ravel()])
            assert np.add.accumulate(shifted, dtype=F32)[-1] == r.total


def test_tie_binades():
    """A byte value ties in exactly one binade, at most 6 except for 255 (binade 24): ties need a small accumulator."""
    table = {k: cc.tie_binade(k) for k in range(1, 256)}
    assert table[255] == 24 and max(v for k, v in table.items() if k != 255) == 6
    assert {k for k, v in table.items() if 3 <= v <= 6} == set(cc.TIE_RICH)
    for k, e in table.items():  # against the definition
        x = np.float64(F32(k) / F32(255))
        for ee in range(-8, 32):
            q = x / 2.0 ** (ee - 23)
            assert (q - np.floor(q) == 0.5) == (ee == e), (k, ee)


def test_walk_lanes():
    lanes, trips, left = set(), set(), set()
    for name in by_group(1):
        for r in reports(name):
            crossing = ~r.headed & (r.ncross > 0) & (r.ntie == 0)
            lanes |= set(r.lane[crossing].tolist())
            trips |= set(r.trip[crossing].tolist())
            assert r.drilled[-1] != r.nchunk - 1 and (r.ncross[-1] > 0)  # the last drill is a crossing's, not the frame's end
            left.add(r.left_after)
    assert {0, 1, 63} <= lanes
    assert max(trips) >= 1
    assert {1, 63, 64, 65} <= left
    assert {cc.case(n).u8.shape[1] % 8 for n in by_group(1)} >= {0, 1}


def test_drill_positions():
    (name,) = by_group(2)
    plain, headed_pos, double = set(), set(), 0
    for r in reports(name):
        ck, th, px = r.where(r.cross)
        headed_chunks = set(r.drilled[r.headed].tolist())
        for c, t, p in zip(ck.tolist(), th.tolist(), px.tolist()):
            (headed_pos if c in headed_chunks else plain).add((t, p))
        key = r.cross // cc.DRILL_PER
        double += int((np.bincount(key - key.min()) >= 2).any()) if key.size else 0
    assert {(0, 0), (63, 15), (64, 0), (1023, 15)} <= plain
    assert any(t == cc.HEAD // cc.DRILL_PER for t, _ in headed_pos)  # the first thread behind the head
    assert double >= 1
    # ... and one of those double crossings in a chunk without a head
    r = cc.report(name, 1)
    ck, th, _ = r.where(r.cross)
    assert any(c not in set(r.drilled[r.headed].tolist()) and np.sum((ck == c) & (th == t)) >= 2 for c, t in zip(ck, th))


def test_several_binades_in_one_chunk():
    (name,) = by_group(3)
    rs = reports(name)
    assert any((r.ncross == 2).any() for r in rs)  # the e + 1 sums of the pass used
    assert any((r.ncross >= 3).any() for r in rs)  # a new pass
    assert any((r.ncross[~r.headed] >= 3).any() for r in rs) and any((r.ncross[r.headed] >= 3).any() for r in rs)
    gains = set()
    for r in rs:
        ok = ~r.headed & r.walked_next  # reached by the walk (which prefetches v_pre), the walk goes on behind it
        gains |= set(np.minimum(r.gain[ok], 2).tolist())
    assert gains == {0, 1, 2}


def test_exact_landings():
    r = cc.report("landings_128", 0)
    assert r.npx == 128 * 128 and r.total == F32(16384) and r.cross[-1] == r.npx - 1 and r.landing.all() and r.cross.size == 14
    natural = {1, 3, 7, 15}
    seen = set()
    for r in reports("landings_shifted"):
        assert r.landing.all() and r.cross.size >= 14
        _, _, px = r.where(r.cross)
        seen |= set(px.tolist())
        assert (~r.headed & (r.ncross > 0)).any()  # landings found by the walk's S + incl == 2^24 too
    assert seen - natural


def test_ties_past_the_head():
    for name in by_group(5):
        for r in reports(name):
            out = ~r.tie_in_head
            assert out.sum() >= 16
            assert (r.tie_up[out]).sum() >= 4 and (~r.tie_up[out]).sum() >= 4
            assert np.unique(r.tie[out] // cc.CHUNK).size >= 3
            assert ((r.ncross == 0) & (r.ntie > 0) & ~r.headed).any()  # drilled for a tie alone
            first = r.drilled[0] * cc.CHUNK
            assert not cc.case(name).u8.reshape(-1, 3)[first : first + cc.HEAD].any()  # the content starts behind the head


def test_tiny_accumulator():
    (name,) = by_group(6)
    for r in reports(name):
        assert r.headed.sum() >= 4 and (r.ncross[:3] == 0).all() and (r.gain[:3] == 0).all()  # below 0.25 across several chunks
        last = r.headed.nonzero()[0][-1]
        assert r.ncross[last] >= 1  # ... then past it inside a headed chunk,
        assert (r.cross % cc.CHUNK >= cc.HEAD).all()  # behind the head
    px = cc.case(name).u8.reshape(-1, 3)[: 4 * cc.CHUNK]
    assert px.max() <= 3 and px.any()


def test_frame_tails():
    seen = set()
    for name in by_group(7):
        u8 = cc.case(name).u8
        npx = u8.shape[0] * u8.shape[1]
        seen.add(npx % cc.CHUNK)
        rs = reports(name)
        assert rs[0].drilled[-1] == rs[0].nchunk - 1 and not rs[0].headed[-1] and rs[0].ncross[-1] == 1  # a crossing in the tail
        assert rs[2].drilled[-1] == rs[2].nchunk - 1 and rs[2].headed[-1] and u8[-1, -1, 2] != 0  # a head that is the tail
    assert seen == {0, 1, 15, 16, 17}
    assert any(cc.case(n).u8.shape[0] * cc.case(n).u8.shape[1] % 4 for n in by_group(7))


def test_saturation():
    H, W = cc.SAT_SHAPE
    npx = H * W
    assert (1 << 24) < npx < (1 << 24) + 2 * cc.CHUNK
    want = F32(np.float64(1 << 24) / npx)
    assert want == F32(0.9992681)
    rs = reports("saturation")
    for r in rs:
        assert r.total == F32(1 << 24) and r.mean == want
    assert rs[0].tie.size == npx - (1 << 24) and not rs[0].tie_up.any()  # every pixel behind 2^24 ties and is rounded away
    assert rs[0].ntie[-1] == npx - (1 << 24)
    assert rs[1].tie.size <= 1  # 254 / 255 is less than half an ulp there
    late = rs[2].tie > (1 << 24)
    assert late.sum() > 1000 and not rs[2].tie_up[late].any()  # its 255s tie, its 254s add nothing


def test_threshold_frames():
    assert len(set(cc.threshold_triple())) == 3  # found by the search in cast_cases, not stated
    t = cc.T05
    for ch, tag in ((1, "green"), (2, "blue")):
        diffs = []
        for which in ("below", "at", "above"):
            name = f"threshold_{tag}_{which}"
            m = cc.sequential_mean(name)
            assert m[0] == 0 and m[3 - ch] == 0
            diffs.append(m[ch] - m[0])
        assert all(d.dtype == F32 for d in diffs)
        assert diffs[0] == np.nextafter(t, F32(0)) and diffs[1] == t and diffs[2] == np.nextafter(t, F32(1))


def test_threshold_kinds_by_the_oracle():
    """The stated kinds are the oracle's.  `at` records the comparison rule of the installed NumPy: a float32 scalar against
    the Python float 0.05 compares in float32 (NEP 50), where float32(0.05) > 0.05 is False; in float64 it would be True."""
    for name, kind in cc.KINDS.items():
        assert cc.classify(cc.case(name).u8) == kind, name
    assert not (cc.T05 > 0.05)
    assert np.float64(cc.T05) > 0.05  # the float64 comparison would call the `at` frames greenish / bluish
    m = cc.sequential_mean("equal_gb")
    assert m[1] == m[2] and m[1] - m[0] > cc.T05
    m = cc.sequential_mean("equal_gb_plus")
    assert m[2] == np.nextafter(m[1], F32(1)) or m[2] > m[1]
    m = cc.sequential_mean("equal_gr")
    assert m[0] == m[1] and m[1] > m[2]


def test_threshold_pairs_at_pipeline_size():
    for kind, ch in (("greenish", 1), ("bluish", 2)):
        a, b = cc.case(f"pair_{kind}_normal").u8, cc.case(f"pair_{kind}_cast").u8
        assert a.shape == cc.PIPE_SHAPE + (3,) and a.shape[1] % 8 == 0 and (a.shape[0] + 1) // 2 * (a.shape[1] // 2) > 8192
        d = b.astype(int) - a.astype(int)
        assert np.count_nonzero(d) == 1 and d.sum() == 1 and np.count_nonzero(d[:, :, ch]) == 1  # one pixel, one level
        ma, mb = cc.sequential_mean(f"pair_{kind}_normal"), cc.sequential_mean(f"pair_{kind}_cast")
        assert ma[ch] - ma[0] <= cc.T05 < mb[ch] - mb[0]
        assert mb[ch] > mb[3 - ch] > mb[0]


def test_seven_chunk_frames():
    names = by_group(11)
    assert len(names) == 5
    frames = [cc.case(n).u8 for n in names]
    assert len({f.shape for f in frames}) == 1 and len({f.tobytes() for f in frames}) == 5
    assert all(cc.report(n, 0).nchunk == 7 for n in names)  # 35 chunks: blocks of 16 chunks end inside frames 2 and 4


def test_fused_shapes():
    for name, (H, W) in zip(by_group(12), cc.FUSED_SHAPES):
        u8 = cc.case(name).u8
        assert u8.shape == (H, W, 3) and W % 8 == 0 and 64 <= W <= cc.CHUNK and ((H + 1) // 2) * ((W + 1) // 2) > 8192
    assert cc.FUSED_SHAPES[0][1] == cc.CHUNK and cc.FUSED_SHAPES[1][1] == 64
    assert cc.FUSED_SHAPES[2][0] % 2 == 1 and cc.FUSED_SHAPES[2][1] % 16 == 8


def test_the_table_covers_every_path():
    lanes, threads, pixels, up, gains = set(), set(), set(), set(), set()
    for name in cc.NAMES:
        for r in reports(name):
            reached = ~r.headed
            lanes |= set(r.lane[reached].tolist())
            plain = np.isin(r.cross // cc.CHUNK, r.drilled[reached])
            _, th, px = r.where(r.cross[plain])
            threads |= set(th.tolist())
            pixels |= set(px.tolist())
            up |= set(r.tie_up[~r.tie_in_head].tolist())
            gains |= set(np.minimum(r.gain[reached], 2).tolist())
    assert {0, 1, 63} <= lanes
    assert {0, 63, 64, 1023} <= threads
    assert {0, 15} <= pixels
    assert up == {True, False}
    assert gains == {0, 1, 2}


def test_general_float_images_are_not_byte_images():
    imgs = cc.general_float_images()
    assert {(5, 7), (300, 400)} <= {v.shape[:2] for v in imgs.values()}
    for name, x in imgs.items():
        assert x.dtype == F32 and x.min() >= 0 and x.max() < 1.06
        assert not np.array_equal((x * 255).astype(np.uint8).astype(F32) / F32(255), x), name
    s = imgs["subnormals_120x160"]
    tiny = np.finfo(F32).tiny
    assert ((s > 0) & (s < tiny)).sum() > 1000 and (s == 0).sum() > 1000
