"""The percentile selection (k_select.hip) against NumPy, bit for bit, on every route.

The selection is exact by design, so each case has one right answer: NumPy 2.2.6's (tests/select_ref.py).
  A. The generic key-digit passes, direct (uwie_percentiles_f32 / uwie_percentiles_f64, HWC): planes of 1 .. 16.8 M
     values, 1 .. 40 images (blocks past the end of tiny planes), constant / two-valued / signed-zero / subnormal / infinite /
     adjacent-ulp / tied values, the eight-group case (every later pass with ng > 4), one plane past 2^24 values.
  B. The pipeline's routes (uwie_enhance_percentiles after uwie_enhance_u8 / uwie_enhance_u8_f64), under every tuning
     that picks a route, against np.percentile of the oracle's restored image (gf_exact = 1: the device's transmission is
     the oracle's, bit for bit).
  C. The DifferentiableEnhancement ranks (stretch and gated modules): the order statistics they save and the forward.
Sensitivity: each of these value-only changes of k_select.hip fails the test named after it -- block_find_digit with
`excl < rank` (test_direct_tiny_and_odd_planes), sel_count without its ng > 4 loop (test_direct_eight_groups),
percentile_indices in double for float32 (test_direct_plane_past_2_24), k_lin_scan answering bin kLinBins - 1 with 0
(test_routes_mixed_batch), the last k_sel_pass writing prefix ^ 1 for odd queries (test_direct_tiny_and_odd_planes), and
k_pct_finish_chain reading o[i] for o[4 + i] (test_routes_select_frames).
NaN inputs are out of scope (np.percentile's result then depends on where its sort puts them).  Signed zeros: NumPy's
sort does not order -0.0 against +0.0, so for planes that mix them the value is compared with NumPy's and the sign with
the total order of the float bits (-0.0 < +0.0), which the key-digit select follows.
"""
import numpy as np
import pytest
import torch

import select_ref as sr

pytestmark = pytest.mark.gpu

QSETS = ((50,), (0, 100), (1e-7, 2.5, 99.999), (2.5, 50, 97.5, 100))


@pytest.fixture(scope="module")
def uw():
    import underwater_image_enhancement_amd as uw

    return uw


@pytest.fixture(scope="module")
def dev(uw):
    return uw.get_device()


@pytest.fixture(scope="module")
def orc():
    from oracle import uwie_oracle

    return uwie_oracle


def device_pct(dev, img, qs):
    t = dev.tensor(img)
    out = dev.percentiles_f32(t, qs) if img.dtype == np.float32 else dev.percentiles_f64(t, qs)
    return out.cpu().numpy()


def key_order_pct(img, qs):
    """np.percentile's arithmetic on the planes sorted by the total order of the float bits (-0.0 < +0.0)."""
    p = sr.planes(img)
    u = np.uint32 if p.dtype == np.float32 else np.uint64
    sign = u(1) << u(8 * p.dtype.itemsize - 1)
    bits = p.view(u)
    keys = np.where(bits & sign, ~bits, bits | sign)
    out = np.empty(p.shape[:2] + (len(qs),), p.dtype)
    for b in range(p.shape[0]):
        for c in range(3):
            s = p[b, c][np.argsort(keys[b, c], kind="stable")]
            for j, q in enumerate(qs):
                prev, nxt, g = sr.percentile_indices(s.size, q, p.dtype)
                out[b, c, j] = sr.lerp(s[prev], s[nxt], g)
    return out


def value_sets(rng, B, H, W, dtype):
    """Named [B, H, W, 3] images of the value patterns selection kernels get wrong."""
    dt = np.dtype(dtype)
    u = np.uint32 if dt == np.float32 else np.uint64
    shape = (B, H, W, 3)
    n = B * H * W * 3
    sets = {"constant": np.full(shape, 0.375, dt),
            "two_values": rng.choice(np.array([-1.5, 2.25], dt), shape)}
    sets["signed_zeros"] = rng.choice(np.array([-0.0, 0.0], dt), shape)
    tiny = np.finfo(dt).smallest_subnormal
    special = np.array([tiny, 3 * tiny, -tiny, np.finfo(dt).tiny, -np.inf, np.inf, -np.finfo(dt).max, -1e30, 1.0, -2.0], dt)
    sets["specials"] = rng.choice(special, shape)
    # runs of consecutive bit patterns across a last-digit boundary (10 bits float32, 9 bits float64): neighbouring ranks
    # differ in the last key digit only
    base = np.array([0.7], dt).view(u)[0] & ~u(1023)
    ulps = (base - u(700) + rng.integers(0, 1400, n).astype(u)).view(dt)
    ulps[rng.random(n) < 0.2] *= -1  # and their negatives: the flipped key order
    sets["adjacent_ulps"] = ulps.reshape(shape)
    ties = rng.choice(np.array([0.1, 0.2, 0.3], dt), shape, p=[0.45, 0.1, 0.45])  # heavy runs straddle the ranks
    few = rng.random(n) < 0.05
    ties.reshape(-1)[few] = rng.random(int(np.count_nonzero(few))).astype(dt)
    sets["ties"] = ties
    return sets


def check_direct(dev, img, qs, what):
    got = device_pct(dev, img, qs)
    with np.errstate(all="ignore"):
        want = sr.percentiles(img, qs)
    sr.assert_same(got, want, what)


TINY = ((1, 1), (1, 2), (1, 3), (2, 2), (1, 5), (7, 9))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_direct_tiny_and_odd_planes(dev, dtype):
    """Planes of 1 .. 63 values, one image (one block) and 40 images (cdiv(256, 120) blocks per plane: most of them past
    the end of the plane, lo == hi, still taking the ticket), and 83 x 129 x 2, through every value pattern."""
    rng = np.random.default_rng(1)
    shapes = [(B, H, W) for H, W in TINY for B in (1, 40)] + [(2, 83, 129)]
    for B, H, W in shapes:
        for name, img in value_sets(rng, B, H, W, dtype).items():
            for qs in QSETS:
                what = f"{np.dtype(dtype).name} {B}x{H}x{W} {name} q={qs}"
                if name == "signed_zeros":
                    got = device_pct(dev, img, qs)
                    assert (got == sr.percentiles(img, qs)).all(), what  # the value: NumPy's
                    sr.assert_same(got, key_order_pct(img, qs), what + " (sign: -0.0 < +0.0)")
                else:
                    check_direct(dev, img, qs, what)
    assert dev.check_status() == 0


def eight_group_plane(rng, n, qs, dtype):
    """A plane whose 2 * len(qs) ranks lie in distinct top-digit buckets (factors of 4 apart: distinct first key digits in
    float32 and float64), so every later pass counts for up to eight groups (sel_count's ng > 4 branch)."""
    ranks = []
    for q in qs:
        prev, nxt, _ = sr.percentile_indices(n, q, dtype)
        ranks += [prev, nxt]
    assert len(set(ranks)) == len(ranks)
    e = np.searchsorted(np.sort(ranks), np.arange(n), side="right")  # bucket of sorted position k: target ranks <= k
    v = (np.float64(4.0) ** (e - 4)) * (1 + 0.5 * np.sort(rng.random(n)))
    return rng.permutation(v.astype(dtype))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_direct_eight_groups(dev, dtype):
    rng = np.random.default_rng(2)
    qs = (2.5, 30, 60, 97.5)
    for B, H, W in ((1, 61, 83), (3, 250, 301)):
        n = H * W
        img = np.stack([np.stack([eight_group_plane(rng, n, qs, dtype) for _ in range(3)], -1) for _ in range(B)])
        img = img.reshape(B, H, W, 3)
        os_ = sr.order_stats(img, qs)
        tops = np.unique(np.floor(np.log(os_.astype(np.float64)) / np.log(4.0)))
        assert tops.size == 8  # the eight ranks really are eight buckets apart
        check_direct(dev, img, qs, f"{np.dtype(dtype).name} {B}x{H}x{W} eight groups")
    assert dev.check_status() == 0


def test_direct_large_planes(dev):
    """Many slabs per plane: 1080p x 2 and 4K x 1 float32, an odd 1079 x 1917 float64 plane, adjacent ulps and ties mixed in."""
    rng = np.random.default_rng(3)
    for B, H, W, dt in ((2, 1080, 1920, np.float32), (1, 2160, 3840, np.float32), (1, 1079, 1917, np.float64)):
        img = rng.normal(0.5, 0.2, (B, H, W, 3)).astype(dt)
        flat = img.reshape(-1)
        flat[::3] = np.round(flat[::3], 2)  # heavy ties
        u = np.uint32 if dt == np.float32 else np.uint64
        flat[1::7] = (np.array([0.5], dt).view(u)[0] + rng.integers(0, 3000, flat[1::7].size).astype(u)).view(dt)
        for qs in QSETS:
            check_direct(dev, img, qs, f"{np.dtype(dt).name} {B}x{H}x{W} q={qs}")
    assert dev.check_status() == 0


def test_direct_plane_past_2_24(dev):
    """4100 x 4100 float32: NumPy computes (n - 1) * q in float32, which at q = 2.5 picks rank 420250 where float64 would
    pick 420249.  The device must follow float32 (the values differ at those ranks, so the float64 choice would fail)."""
    rng = np.random.default_rng(4)
    H = W = 4100
    n = H * W
    # value = position for every position below 2^24: neighbouring ranks differ there (uniform float32 draws would tie)
    img = np.stack([rng.permutation(n).astype(np.float32) for _ in range(3)], -1).reshape(1, H, W, 3)
    qs = (2.5, 50, 85, 97.5)
    p32 = sr.percentile_indices(n, 2.5, np.float32)
    p64 = sr.percentile_indices(n, 2.5, np.float64)
    assert p32[0] == 420250 and p64[0] == 420249
    got = device_pct(dev, img, qs)
    want = sr.percentiles(img, qs)
    sr.assert_same(got, want, "4100 x 4100 float32")
    # the float64 index arithmetic gives another answer on this plane: the comparison above can tell them apart
    plane = sr.planes(img)[0, 0]
    v = sr.kth(plane, [p64[0], p64[1]])
    alt = sr.lerp(v[0], v[1], np.float32(p64[2]))
    assert alt != want[0, 0, 0]
    assert dev.check_status() == 0


# ------------------------------------------------------------------ B. pipeline routes
SIX = {1: (0.3, 20, 0.5), 2: (0.5, 15, 0.5), 3: (0.7, 10, 0.1)}  # omega, ksize, eps (six_stadigy.py:230-285)

GRID = (("default", {}), ("rank_sweep2", dict(rank_sweep=2)), ("restore_store", dict(restore_store=1)),
        ("select_generic", dict(select_generic=1)), ("lin_cap16", dict(lin_cap=16)), ("no_predict", dict(lin_no_predict=1)),
        ("shift2", dict(lin_predict_shift=2)), ("shift400", dict(lin_predict_shift=400)), ("predict3", dict(lin_predict3=1)),
        ("streams4_cap16", dict(streams=4, lin_cap=16)))


def reference_pct(orc, u8, key):
    """np.percentile of the oracle's restored image: [3, 2] (strategies 1-2, medium_dehazing) or [3, 4] (strategy 3)."""
    x = orc.normalise_u8(u8)
    if key == "medium_dehazing":
        D = orc.DictStrategyOracle
        A = D.atmosphere(x, 1)
        y = D.recover(x, D.transmission(x, A, omega=0.6, r=20), A)
        return sr.percentiles(y[None], (15, 92))[0].astype(np.float64)
    x = orc.correct_cast(x, orc.classify_cast(x))
    omega, ks, eps = SIX[key]
    y = orc.SixStrategyOracle.dehaze(x, omega, ks, eps)
    if key == 3:
        return sr.chain_percentiles(y[None], 20, 85, 2)[0].astype(np.float64)
    lo, hi = {1: (5, 98), 2: (15, 95)}[key]
    return sr.percentiles(y[None], (lo, hi))[0].astype(np.float64)


def route_params(dev, key, gf_exact=1):
    from underwater_image_enhancement_amd import _lib
    from underwater_image_enhancement_amd.api import _dict_params

    if key == "medium_dehazing":
        p = _dict_params(dev, key, {})
        p.gf_exact = gf_exact
        return p
    return dev.params(_lib.SURFACE_SIX, key, gf_exact=gf_exact)


def route_pct(dev, frames, key, f64=False, gf_exact=1, **params):
    """Percentiles of one enhance call (f64: the dict surface through uwie_enhance_u8_f64, which never splits the batch)."""
    t = torch.from_numpy(np.ascontiguousarray(frames)).to(dev.torch_device)
    p = route_params(dev, key, gf_exact)
    for k, v in params.items():
        setattr(p, k, v)
    enhance = dev.enhance_u8_f64_with_percentiles if f64 else dev.enhance_u8_with_percentiles
    *_, pct = enhance(t, p)
    return pct.cpu().numpy()


# (strategy, entry point): the dict strategy through both uwie_enhance_u8 and uwie_enhance_u8_f64
ROUTE_KEYS = ((1, False), (2, False), (3, False), ("medium_dehazing", False), ("medium_dehazing", True))


def check_routes(dev, orc, frames, tag, cells=GRID, alone=True):
    """Every route key x tuning cell: the batch's percentiles equal the oracle's, and (alone) each frame's run alone."""
    want = {k: np.stack([reference_pct(orc, f, k) for f in frames]) for k in (1, 2, 3, "medium_dehazing")}
    for cell, tuning in cells:
        with dev.tuning(**tuning):
            for k, f64 in ROUTE_KEYS:
                what = f"strategy {k}{' (f64 entry)' if f64 else ''} [{cell}]"
                sr.assert_same(route_pct(dev, frames, k, f64), want[k], f"{tag} {what}")
                if alone and len(frames) > 1:
                    for i, f in enumerate(frames):
                        sr.assert_same(route_pct(dev, f[None], k, f64)[0], want[k][i], f"{tag} frame {i} alone, {what}")
        assert dev.check_status() == 0, cell


def test_routes_select_frames(dev, orc):
    from test_gpu_enhance import select_frames

    for name, u8 in zip(("noisy", "flatish", "odd", "wide", "big"), select_frames()):
        check_routes(dev, orc, u8[None], name)


def mixed_batch():
    """The batch of test_select_flagged_planes_in_a_split_batch: a constant frame (every plane flags under lin_cap = 16),
    a black-and-white checker (restores to exact 0 and 1: answered by the scans), crops of the select frames."""
    from test_gpu_enhance import select_frames

    noisy, flatish, odd, wide, big = select_frames()
    flat = np.empty((120, 200, 3), np.uint8)
    flat[:] = (90, 140, 180)
    yy, xx = np.mgrid[0:120, 0:200]
    checker = np.repeat((((yy // 20) + (xx // 20)) % 2 * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    return np.stack([flat, noisy[:120, :200], checker, big[200:320, 300:500], odd[:120, :200], wide[100:220, 400:600],
                     flatish[150:270, 60:260], flatish[:120, :200]])


def test_routes_mixed_batch(dev, orc):
    check_routes(dev, orc, mixed_batch(), "mixed 8 x 120 x 200")


def hd_frames(rng, B, H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for b in range(B):
        f = np.stack([30 + 0.05 * xx + 0.03 * yy + 10 * b, 90 + 0.02 * xx, 180 - 0.04 * yy], -1) + rng.normal(0, 14, (H, W, 3))
        out.append(np.clip(f, 0, 255).astype(np.uint8))
    return np.stack(out)


def test_routes_1080p(dev, orc):
    check_routes(dev, orc, hd_frames(np.random.default_rng(5), 1, 1080, 1920), "1080p")


def test_routes_4k_batch(dev, orc):
    """4K x 3 = 24.9 M pixels: strategies 1-2 take the rank-counting route by default (4K x 2 would stay under 2^24).
    The whole grid, and every frame alone.  A batch of three is not split by streams = 4 (uwie_enhance_u8 splits only
    batches of at least `streams` frames), so one more cell splits it three ways."""
    frames = hd_frames(np.random.default_rng(6), 3, 2160, 3840)
    assert frames.shape[0] * 2160 * 3840 >= 2**24
    check_routes(dev, orc, frames, "4K x 3", GRID + (("streams3_cap16", dict(streams=3, lin_cap=16)),))


def test_f32t_routes_agree(dev):
    """UWIE_INTER_F32T has no oracle: its recomputing routes (the histogram sweep, the recomputed float32 fallback of the
    planes lin_cap = 16 flags) and the stored planes select over the same float32 values (restore.h one32_raw).  The float32
    transmission exists only without gf_exact (the exact-order filter writes float64) and for even widths (W = 200 here);
    that it was taken shows in the percentiles, which differ from INTER_F64's on these frames."""
    from underwater_image_enhancement_amd import _lib

    frames = mixed_batch()
    assert frames.shape[2] % 2 == 0
    for k in (1, 2, 3):
        with dev.tuning(restore_store=1):
            want = route_pct(dev, frames, k, gf_exact=0, inter_dtype=_lib.INTER_F32T)
            f64 = route_pct(dev, frames, k, gf_exact=0, inter_dtype=_lib.INTER_F64)
        assert not sr.same_bits(want, f64).all(), f"strategy {k}: INTER_F32T gave INTER_F64's percentiles"
        for tuning in ({}, dict(rank_sweep=2), dict(lin_cap=16), dict(lin_cap=16, streams=4)):
            with dev.tuning(**tuning):
                got = route_pct(dev, frames, k, gf_exact=0, inter_dtype=_lib.INTER_F32T)
                sr.assert_same(got, want, f"F32T strategy {k} {tuning}")
    assert dev.check_status() == 0


# ------------------------------------------------------------------ C. DifferentiableEnhancement ranks
def diff_cases():
    """(H, W): planes not a multiple of 4 values (planar: misaligned channel planes, the scalar path) and multiples of 4
    (the 16-byte path with slab tails); 1 x 1 (n = 1)."""
    return ((1, 1), (5, 7), (13, 11), (16, 20), (33, 36), (64, 100), (127, 129))


def L_pairs():
    """L values at 0 / 100, where (L / 100.0) * n lands on an integer, and one float32 ulp below those."""
    below = lambda v: float(np.nextafter(np.float32(v), np.float32(0)))  # noqa: E731
    return [(0.0, 100.0), (25.0, 75.0), (below(25.0), below(75.0)), (50.0, below(100.0)), (below(50.0), 100.0)]


@pytest.mark.parametrize("planar", [0, 1])
def test_diff_enhance_ranks(dev, planar):
    from diffenh_grad_ref import diff_enhance

    rng = np.random.default_rng(7)
    for H, W in diff_cases():
        n = H * W
        pairs = L_pairs()
        B = len(pairs)
        img = rng.permutation(np.arange(B * 3 * n, dtype=np.float32)).reshape(B, 3, H, W) / np.float32(B * 3 * n)  # distinct
        x = img if planar else np.ascontiguousarray(img.transpose(0, 2, 3, 1))
        params = np.array([[lo, hi, 0, 1] for lo, hi in pairs], np.float32)
        out, saved = dev.diff_enhance_save_f32(dev.tensor(x), dev.tensor(params), bool(planar), 0)
        out, saved = out.cpu().numpy(), saved.cpu().numpy()
        want_saved = np.empty((B, 3, 2), np.float32)
        klo, khi = sr.stretch_positions(params[:, 0], n), sr.stretch_positions(params[:, 1], n)
        for b in range(B):
            for c in range(3):
                want_saved[b, c] = sr.kth(img[b, c], [klo[b], khi[b]])
        sr.assert_same(saved, want_saved, f"stretch {H}x{W} planar={planar}")
        want = diff_enhance(torch.from_numpy(x), torch.from_numpy(params[:, :1]), torch.from_numpy(params[:, 1:2]),
                            None, None, planar=bool(planar)).numpy()
        sr.assert_same(out, want, f"stretch forward {H}x{W} planar={planar}")
    assert dev.check_status() == 0


@pytest.mark.parametrize("planar", [0, 1])
def test_diff_gated_ranks(dev, planar):
    from dlp_grad_ref import gated

    rng = np.random.default_rng(8)
    for H, W in diff_cases():
        n = H * W
        pairs = [(lo, hi if hi < 100 else float(np.nextafter(np.float32(100), np.float32(0)))) for lo, hi in L_pairs()]
        B = len(pairs)
        img = rng.permutation(np.arange(B * 3 * n, dtype=np.float32)).reshape(B, 3, H, W) / np.float32(B * 3 * n)
        x = img if planar else np.ascontiguousarray(img.transpose(0, 2, 3, 1))
        params = np.array([[lo, hi, 0, 1] for lo, hi in pairs], np.float32)  # use_gamma = 0: the stretch alone
        out, saved = dev.diff_gated_save_f32(dev.tensor(x), dev.tensor(params), bool(planar))
        out, saved = out.cpu().numpy(), saved.cpu().numpy()
        klo, khi = sr.gated_positions(params[:, 0], n), sr.gated_positions(params[:, 1], n)
        want_saved = np.empty((B, 3, 2), np.float32)
        for b in range(B):
            for c in range(3):
                want_saved[b, c] = sr.kth(img[b, c], [klo[b], khi[b]])
        sr.assert_same(saved, want_saved, f"gated {H}x{W} planar={planar}")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
        want = gated(t(x), t(params[:, :1]), t(params[:, 1:2]), t(params[:, 2:3]), t(params[:, 3:4]), planar=bool(planar)).numpy()
        sr.assert_same(out, want, f"gated forward {H}x{W} planar={planar}")
    assert dev.check_status() == 0


# ------------------------------------------------------------------ D. the host path: tiny planes, launches per route
def test_routes_tiny_planes(dev, orc):
    """Planes of 1 .. 24 pixels through every route key and tuning cell: fewer than four pixels is where no sample is drawn
    (ngroups == 0) and where the rank route's npx >= 4 guard sits; 1 x 5 and 3 x 8 have a ragged and a whole last group of
    four.  One batch of two frames as well."""
    rng = np.random.default_rng(9)
    for H, W in ((1, 1), (1, 3), (2, 2), (1, 5), (3, 8)):
        frame = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        check_routes(dev, orc, frame[None], f"tiny {H}x{W}", alone=False)
    check_routes(dev, orc, rng.integers(0, 256, (2, 3, 8, 3), dtype=np.uint8), "tiny 2 x 3x8", alone=False)


ROW_PREFIXES = ("k_sel_", "k_lin_", "k_rank_", "k_restore_", "k_recover64_", "k_pct_")
ROW_CELLS = (("default", {}), ("rank_sweep2", dict(rank_sweep=2)), ("restore_store", dict(restore_store=1)),
             ("select_generic", dict(select_generic=1)), ("no_predict", dict(lin_no_predict=1)), ("lin_cap16", dict(lin_cap=16)))
ROW_ROUTES = ((2, False), (3, False), ("medium_dehazing", False), ("medium_dehazing", True))


def selection_rows(dev, frames):
    """{(cell, strategy, f64 entry): {profiler row name: launches}} of the selection's and its producers' kernels (a launch
    of a kernel with two template arguments is reported in parentheses: "(k_lin_collect_src<float, 4>)")."""
    out = {}
    for cell, tuning in ROW_CELLS:
        with dev.tuning(**tuning):
            for k, f64 in ROW_ROUTES:
                dev.profile(True)
                try:
                    route_pct(dev, frames, k, f64)
                    rows = dev.profile_rows()
                finally:
                    dev.profile(False)
                out[cell, k, f64] = {name: calls for name, (_, calls) in sorted(rows.items()) if name.lstrip("(").startswith(ROW_PREFIXES)}
    return out


# Recorded by running selection_rows at the commit before the float32 and float64 host paths were merged (never from the
# merged code): bench.py and profiles/f32t_stats.py match rows by these names.  Which kernels are launched and how often is
# decided on the host (shape, tuning, strategy), never by the data.  Every row is one launch, but the key-digit passes': one
# per digit (three float32, six float64), which return at once for planes that are not flagged.
def _rows(passes, *names):
    return {**{name: 1 for name in names}, "k_sel_pass<Src>": passes}


LIN32 = ("k_lin_predict", "k_lin_scan<float>", "k_lin_finish<float>", "k_restore_hist_collect", "k_pct_finish<V>")
LIN32_S3 = ("k_lin_predict", "k_lin_scan<float>", "k_lin_finish<float>", "k_restore_hist_collect4", "k_lin_collect<float>",
            "k_pct_finish_chain")  # strategy 3: no sample, four windows, stored planes, the chained finish
LIN64 = ("k_lin_predict", "k_lin_scan<double>", "k_lin_finish<double>", "k_recover64_hist_collect", "k_pct_finish<V>")
RANK32 = ("k_lin_predict", "k_lin_sample<float>", "k_restore_rank", "k_rank_scan", "k_lin_finish<float>", "k_pct_finish<V>")
SRC32, SRC64 = "(k_lin_collect_src<float, 4>)", "k_lin_collect_src64"
ROWS_BY_CELL = {  # cell: strategy 2, strategy 3, medium_dehazing (the same through both entry points)
    "default": (_rows(3, *LIN32, "k_lin_sample<float>", SRC32), _rows(3, *LIN32_S3), _rows(6, *LIN64, "k_lin_sample<double>", SRC64)),
    "rank_sweep2": (_rows(3, *RANK32), _rows(3, *LIN32_S3), _rows(6, *LIN64, "k_lin_sample<double>", SRC64)),
    "restore_store": (_rows(3, *LIN32, "k_lin_sample<float>", "k_lin_collect<float>"), _rows(3, *LIN32_S3),
                      _rows(6, *LIN64, "k_lin_sample<double>", "k_lin_collect<double>")),
    "select_generic": (_rows(3, "k_sel_init<K>", "k_restore_hist_key", "k_pct_finish<V>"),
                       _rows(3, "k_sel_init<K>", "k_restore_hist_key", "k_pct_finish_chain"),
                       _rows(6, "k_sel_init<K>", "k_recover64_hist_key", "k_pct_finish<V>")),
    "no_predict": (_rows(3, *LIN32, SRC32), _rows(3, *LIN32_S3), _rows(6, *LIN64, SRC64)),
    "lin_cap16": (_rows(3, *LIN32, "k_lin_sample<float>", SRC32), _rows(3, *LIN32_S3), _rows(6, *LIN64, "k_lin_sample<double>", SRC64)),
}
ROWS = {(cell, k, f64): by[min(i, 2)] for cell, by in ROWS_BY_CELL.items() for i, (k, f64) in enumerate(ROW_ROUTES)}


def test_profiler_rows_per_route(dev):
    frames = np.random.default_rng(10).integers(0, 256, (2, 48, 64, 3), dtype=np.uint8)
    got = selection_rows(dev, frames)
    assert sorted(got, key=str) == sorted(ROWS, key=str)
    for key in ROWS:
        assert got[key] == ROWS[key], f"{key}: {got[key]}"
    assert dev.check_status() == 0
