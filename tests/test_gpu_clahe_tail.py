"""CLAHE's three device implementations against the oracle on the cases of tests/clahe_cases.py: tile grids away from 8 x 8,
clip limits from none to every-count-clipped, rounding ties, and the launch routes that the usual frame sizes never take.

  stage kernels   k_clahe_lut / k_clahe_apply (k_clahe.hip): uwie_clahe_u8, uwie_clahe_f32, dict clahe_enhancement on a
                  general float32 / float64 image
  fused tail      k_stretch_lab_lut<0|1> (256 threads, or the 1024-thread wide form) + k_clahe_apply_u8 / _f32 (k_fused.hip):
                  strategies 1 and 2, recomputed source and stored planes (tuning restore_store), float image wanted or not
  code domain     k_stretch_lab_lut<2> + k_clahe_apply_codes: strategies 4, 5, 6 and dict clahe_enhancement on a u8-derived image

The reference is the oracle's own composition (SixStrategyOracle.strategy / DictStrategyOracle.run) with the case's grid and
clip limit.  Bounds, the project's standing ones: without pow (strategy 2; dict clahe_enhancement with apply_gamma off) every
byte and every float equal; with pow (strategies 1, 4, 5, 6) at most 1 LSB, the count printed.  The dehazing strategies run
with gf_exact = 1: the fused guided filter's 1e-11 on t is pinned elsewhere.  tests/test_clahe_cases.py holds the
preconditions (and the oracle's CLAHE against a second restatement) on the CPU.
"""
import ctypes

import numpy as np
import pytest

import clahe_cases as C
import clahe_ref as R

pytestmark = pytest.mark.gpu

IDS = [c.id for c in C.CASES]
POW = {1: True, 2: False, 4: True, 5: True, 6: True}


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


def over(case, dehaze):
    o = dict(tiles_x=case.tiles[0], tiles_y=case.tiles[1], clip_limit=case.clip)
    if dehaze:
        o["gf_exact"] = 1
    return o


def same(got, want, tag):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, want.dtype, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got.ravel() != want.ravel())
        where = np.unravel_index(bad[0], got.shape)
        raise AssertionError(f"{tag}: {bad.size} of {got.size} differ; first at {where}: got {got.ravel()[bad[0]]!r} "
                             f"want {want.ravel()[bad[0]]!r}")


def bytes_ok(got, want, tag, pow_):
    """Equal without pow; at most 1 LSB with it (the count printed)."""
    if not pow_:
        return same(got, want, tag)
    assert got.dtype == want.dtype == np.uint8 and got.shape == want.shape, tag
    d = np.abs(got.astype(np.int16) - want.astype(np.int16))
    print(f"{tag}: {np.count_nonzero(d)} of {d.size} bytes differ by 1 LSB")
    assert d.max(initial=0) <= 1, f"{tag}: max |delta| = {d.max()} LSB ({np.count_nonzero(d > 1)} bytes beyond 1)"


def six_float(orc, u8, k, case):
    """The float32 image of strategy k as enhance_u8 sees it (cast detection on), at the case's grid and clip limit."""
    x = orc.normalise_u8(u8)
    x = orc.correct_cast(x, orc.classify_cast(x))
    return orc.SixStrategyOracle.strategy(k, x, case.tiles, case.clip)


def clahe_input_L(orc, u8, k):
    """The L plane strategy k hands to CLAHE."""
    x = orc.normalise_u8(u8)
    x = orc.correct_cast(x, orc.classify_cast(x))
    y = orc.SixStrategyOracle.before_clahe(k, x)
    return np.ascontiguousarray(orc.cv_rgb2lab_u8((y * 255).astype(np.uint8))[:, :, 0])


def assert_ties(orc, u8, k, case):
    if case.group == "ties":
        ref = R.clahe(clahe_input_L(orc, u8, k), case.clip, case.tiles)
        assert ref.lut_ties > 0 and ref.blend_ties > 0, (case.id, k, ref.lut_ties, ref.blend_ties)


# ------------------------------------------------------------------------------------------------------ stage kernels
@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_stage_kernels(uw, dev, orc, monkeypatch, case):
    u8 = C.case_frame(case)
    plane = np.ascontiguousarray(u8[:, :, 0])
    same(dev.clahe_u8(dev.tensor(plane[None]), case.clip, case.tiles)[0].cpu().numpy(), orc.cv_clahe_u8(plane, case.clip, case.tiles),
         f"{case.id} clahe_u8")
    img = C.general_float(case, np.float32)
    same(dev.clahe_f32(dev.tensor(img[None]), case.clip, case.tiles)[0].cpu().numpy(),
         orc.SixStrategyOracle.clahe(img, case.clip, case.tiles), f"{case.id} clahe_f32")
    monkeypatch.setattr(uw.EnhancementStrategies, "swallow_errors", False)
    params = dict(clip_limit=case.clip, tile_grid_size=case.tiles, apply_gamma=False)
    for dtype in (np.float32, np.float64):
        x = C.general_float(case, dtype)
        with pytest.raises(uw.UnsupportedInputError):
            uw.api._recover_u8(x)  # the general float path, not the code domain
        same(uw.EnhancementStrategies.apply_strategy(x, "clahe_enhancement", params),
             orc.DictStrategyOracle.run(x, "clahe_enhancement", params), f"{case.id} dict clahe_enhancement on general {dtype.__name__}")


# --------------------------------------------------------------------------------------------------------- fused tail
@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_fused_tail(uw, dev, orc, case):
    u8 = C.case_frame(case)
    for k in (2, 1):
        assert_ties(orc, u8, k, case)
        want = orc.enhance_u8(u8, k, tiles=case.tiles, clip=case.clip)
        wantf = six_float(orc, u8, k, case)
        for store in (0, 1):
            with dev.tuning(restore_store=store):
                tag = f"{case.id} strategy {k} restore_store={store}"
                bytes_ok(uw.enhance(u8, strategy=k, **over(case, True)), want, tag + " (k_clahe_apply_u8)", POW[k])
                out, outf = dev.enhance_u8(dev.tensor(u8[None]), dev.params(0, k, **over(case, True)), want_float=True)
                bytes_ok(out[0].cpu().numpy(), want, tag + " (k_clahe_apply_f32)", POW[k])
                gotf = outf[0].cpu().numpy()
                if POW[k]:  # float32 pow: one rounding apart at most, 1.2e-7 below 1.0
                    assert gotf.dtype == np.float32 and np.abs(gotf.astype(np.float64) - wantf).max(initial=0) <= 2e-7, tag
                else:
                    same(gotf, wantf, tag + " float image")


@pytest.mark.parametrize("k", [1, 2])
def test_fused_tail_f32t_keeps_its_contract_at_every_grid(uw, orc, k):
    """inter_dtype = F32T has no oracle of its own and its image before CLAHE is not obtainable, so this is the contract of
    test_f32t_transmission_stated_tolerance against the float64 reference and no more, summed over the cases as that test sums
    over its frames: at least 99.98 % of the bytes identical, at most 5e-5 beyond 1 LSB, none beyond 10, PSNR >= 80 dB."""
    from underwater_image_enhancement_amd import _lib

    tot = diff = beyond = worst = 0
    sq = 0.0
    for case in C.CASES:
        u8 = C.case_frame(case)
        o = over(case, False)
        d = np.abs(uw.enhance(u8, strategy=k, inter_dtype=_lib.INTER_F32T, **o).astype(int)
                   - orc.enhance_u8(u8, k, tiles=case.tiles, clip=case.clip).astype(int))
        if d.any():
            print(f"{case.id}: {np.count_nonzero(d)} bytes differ, worst {d.max()}")
        tot += d.size
        diff += int(np.count_nonzero(d))
        beyond += int(np.count_nonzero(d > 1))
        worst = max(worst, int(d.max()))
        sq += float((d.astype(np.float64) ** 2).sum())
    psnr = 10 * np.log10(255.0 ** 2 * tot / sq) if sq else np.inf
    print(f"inter_dtype=F32T strategy {k}: {diff} of {tot} bytes differ ({beyond} by more than 1 LSB, worst {worst}), PSNR {psnr:.1f} dB")
    assert diff <= 2e-4 * tot and beyond <= 5e-5 * tot and worst <= 10 and psnr >= 80.0, (k, diff, beyond, worst, psnr)


# -------------------------------------------------------------------------------------------------------- code domain
@pytest.mark.parametrize("case", C.CASES, ids=IDS)
def test_code_domain(uw, dev, orc, monkeypatch, case):
    u8 = C.case_frame(case)
    for k in (4, 5, 6):
        assert_ties(orc, u8, k, case)
        tag = f"{case.id} strategy {k}"
        want = orc.enhance_u8(u8, k, tiles=case.tiles, clip=case.clip)
        bytes_ok(uw.enhance(u8, strategy=k, **over(case, False)), want, tag, True)
        out, outf = dev.enhance_u8(dev.tensor(u8[None]), dev.params(0, k, **over(case, False)), want_float=True)
        bytes_ok(out[0].cpu().numpy(), want, tag + " with the float image", True)
        assert np.abs(outf[0].cpu().numpy().astype(np.float64) - six_float(orc, u8, k, case)).max(initial=0) <= 2e-7, tag
    # dict clahe_enhancement on the u8-derived image: tile_grid_size = (tiles_x, tiles_y), as cv2.createCLAHE takes it
    monkeypatch.setattr(uw.EnhancementStrategies, "swallow_errors", False)
    x = orc.normalise_u8(u8)
    ES = orc.DictStrategyOracle
    params = dict(clip_limit=case.clip, tile_grid_size=case.tiles, apply_gamma=False)
    want = ES.run(x, "clahe_enhancement", params)
    tag = f"{case.id} dict clahe_enhancement"
    same(uw.EnhancementStrategies.apply_strategy(x, "clahe_enhancement", params), want, tag + " float64")
    p = uw.api._dict_params(dev, "clahe_enhancement", params)
    assert (p.tiles_x, p.tiles_y) == case.tiles
    out, outf = dev.enhance_u8(dev.tensor(u8[None]), p, want_float=True)
    same(out[0].cpu().numpy(), (want * 255).astype(np.uint8), tag + " bytes")
    same(outf[0].cpu().numpy(), want.astype(np.float32), tag + " float32")
    params["apply_gamma"] = True
    want = ES.run(x, "clahe_enhancement", params)
    got = uw.EnhancementStrategies.apply_strategy(x, "clahe_enhancement", params)
    assert np.abs(got - want).max(initial=0) < 1e-9, tag  # float64 pow: a few ulp between libraries
    bytes_ok((got * 255).astype(np.uint8), (want * 255).astype(np.uint8), tag + " with gamma", True)


# ------------------------------------------------------------------------------------------------------------ batches
@pytest.mark.parametrize("tiles", [(3, 2), (12, 12)])
def test_batch_equals_single_calls(uw, dev, orc, tiles):
    frames = C.batch_frames()
    for k in (1, 2, 4, 5, 6):
        o = dict(tiles_x=tiles[0], tiles_y=tiles[1], **({"gf_exact": 1} if k <= 2 else {}))
        got = uw.enhance(frames, strategy=k, **o)
        for i, u8 in enumerate(frames):
            same(got[i], uw.enhance(u8, strategy=k, **o), f"strategy {k} tiles {tiles}: frame {i} of the batch against its single call")
            bytes_ok(got[i], orc.enhance_u8(u8, k, tiles=tiles), f"strategy {k} tiles {tiles}: frame {i} of the batch", POW[k])
    p = uw.api._dict_params(dev, "clahe_enhancement", dict(tile_grid_size=tiles))
    out, outf = dev.enhance_u8_f64(dev.tensor(frames), p)
    for i, u8 in enumerate(frames):
        one, onef = dev.enhance_u8_f64(dev.tensor(u8[None]), p)
        same(out[i].cpu().numpy(), one[0].cpu().numpy(), f"dict clahe_enhancement tiles {tiles}: frame {i} bytes")
        same(outf[i].cpu().numpy(), onef[0].cpu().numpy(), f"dict clahe_enhancement tiles {tiles}: frame {i} float64")
        same(outf[i].cpu().numpy(), orc.DictStrategyOracle.run(orc.normalise_u8(u8), "clahe_enhancement", dict(tile_grid_size=tiles)),
             f"dict clahe_enhancement tiles {tiles}: frame {i} against the oracle")


def test_fan_out_at_12x12_equals_the_oracle(uw, dev, orc):
    """uwie_enhance_all_u8 with 12 x 12 tiles in every set: one workspace, shared front end, and every CLAHE strategy's plane
    against the oracle (tests/test_gpu_enhance.py compares this grid with the single device call only)."""
    import torch

    from underwater_image_enhancement_amd import _lib

    frames = C.batch_frames()
    B, H, W = frames.shape[:3]
    p6 = (_lib.UwieParams * 6)()
    for k in range(6):
        p6[k] = dev.params(_lib.SURFACE_SIX, k + 1, tiles_x=12, tiles_y=12, **({"gf_exact": 1} if k < 3 else {}))
    need = dev.lib.uwie_workspace_bytes_all(B, H, W, ctypes.cast(p6, ctypes.c_void_p))
    ws = dev.workspace(need)
    out = dev.empty((6, B, H, W, 3), torch.uint8)
    d_in = dev.tensor(frames)
    _lib.check(dev.lib.uwie_enhance_all_u8(dev._ctx, ctypes.c_void_p(d_in.data_ptr()), ctypes.c_void_p(out.data_ptr()), None, B, H, W,
                                           ctypes.cast(p6, ctypes.c_void_p), ctypes.c_void_p(ws.data_ptr()), need, dev.stream()))
    got = out.cpu().numpy()
    dev.check_status()
    for k in (1, 2, 4, 5, 6):
        for i, u8 in enumerate(frames):
            bytes_ok(got[k - 1, i], orc.enhance_u8(u8, k, tiles=(12, 12)), f"fan-out strategy {k} frame {i}", POW[k])
            same(got[k - 1, i], uw.enhance(u8, strategy=k, tiles_x=12, tiles_y=12, **({"gf_exact": 1} if k <= 2 else {})),
                 f"fan-out strategy {k} frame {i} against the single call")


# ------------------------------------------------------------------------------------------------------------- routes
ROUTE_CASES = C.of_group("flat", "wide", "ragged") + [C.BY_ID["grid-96x120-t12x12-c2-underwater"]]


def lut_and_apply_rows(dev):
    rows = dev.profile_rows()
    return sorted(n for n in rows if n.startswith("k_stretch_lab_lut")), sorted(n for n in rows if n.startswith("k_clahe_apply"))


@pytest.mark.parametrize("case", ROUTE_CASES, ids=[c.id for c in ROUTE_CASES])
def test_routes(uw, dev, case):
    """The LUT kernel's form and the apply kernel's variant, read from the context's profiler, against the library's own plan
    (uwie_clahe_plan).  The flat / walk split inside the apply kernel is not visible to a profiler: the plan's cell counts
    stand for it (they come from the kernel's own condition), and tests/test_clahe_cases.py asserts them."""
    from underwater_image_enhancement_amd import _lib

    d_in = dev.tensor(C.case_frame(case)[None])
    plan = _lib.clahe_plan(1, case.H, case.W, case.tiles, case.clip, recomputed=True)
    dev.profile(True)
    try:
        for want_float in (False, True):
            apply_row = ["k_clahe_apply_f32" if want_float else "k_clahe_apply_u8"]
            dev.profile_rows()
            dev.enhance_u8(d_in, dev.params(0, 2, **over(case, True)), want_float=want_float)
            assert lut_and_apply_rows(dev) == (["k_stretch_lab_lut_wide" if plan.wide_lut else "k_stretch_lab_lut<1>"], apply_row), case.id
            with dev.tuning(restore_store=1):  # stored planes: not a recomputed source, never the wide form
                assert _lib.clahe_plan(1, case.H, case.W, case.tiles, case.clip, recomputed=False).wide_lut == 0
                dev.enhance_u8(d_in, dev.params(0, 2, **over(case, True)), want_float=want_float)
                assert lut_and_apply_rows(dev) == (["k_stretch_lab_lut<0>"], apply_row), case.id
        for k in (4, 6):  # CLAHE first (raw codes + histogram) and CLAHE last (final tables): the same two kernels
            dev.enhance_u8(d_in, dev.params(0, k, **over(case, False)))
            assert lut_and_apply_rows(dev) == (["k_stretch_lab_lut<2>"], ["k_clahe_apply_codes"]), (case.id, k)
    finally:
        dev.profile(False)
    if case.group == "wide":
        assert plan.wide_lut == 1
    if case.group == "flat":
        assert plan.cells_flat >= 1 and plan.cells_walk >= 1
