"""Every device restatement of OpenCV's 8-bit RGB <-> LAB and RGB -> gray arithmetic against the oracle, on all 2^24 colours.
The frames and compositions are those of tests/colour_cases.py; tests/test_colour_cases.py holds, on the CPU, what makes them
reach the arithmetic they are aimed at (and prints the coverage).

  stage kernels    rgb2lab_px / lab2rgb_px of k_clahe.hip (table driven): uwie_rgb2lab_u8, uwie_lab2rgb_u8 (out-of-gamut LAB
                   bytes included), uwie_clahe_f32 and the dict surface's general float route on a float cube that is not
                   u8 / 255 data; uwie_rgb2gray_u8 at both shifts
  to_lab           k_stretch_lab_lut<2> (dict clahe_enhancement with L_low 0, L_high 100: no table before LAB, bytes - 1 behind
                   LAB -> RGB; strategy 6 rides along, <= 1 LSB for its pow) and <0> (strategy 2, tuning restore_store = 1)
  lab_of           the fast path of k_stretch_lab_lut<1> and its 1024-thread wide form: strategy 2 with omega 0 and percentiles
                   (0, 99.5) on the four quarters of the shuffled cube, whose bytes reach LAB unchanged
  inline LAB2RGB   k_clahe_apply_u8 / _f32 / _codes on the frames of colour_cases.LAB_FRAMES (>= 3.5 M distinct (L', a, b))
  gray planes      k_quant_gray (uwie_transmission_init) and the quadtree's own (uwie_atmospheric_light, tuning entry_fuse
                   0, 1, 2) for every forced cast kind at gray_shift 14 and 15

The LAB plane of k_stretch_lab_lut is not exposed: a wrong L, a or b shows in the RGB bytes behind LAB -> RGB for >= 99.5 % of
the LAB triples (test_one_step_in_lab_shows_in_the_rgb_bytes), and a wrong L moves the tile histograms besides.
Bounds, the project's standing ones: every byte and every float equal where no pow is involved; <= 1 LSB (2e-7 on the float32
image) for strategy 6."""
import numpy as np
import pytest

import colour_cases as K
from test_gpu_clahe_tail import bytes_ok, lut_and_apply_rows, same

pytestmark = pytest.mark.gpu

ORDERS = ["cube", "shuffled"]
CAST_KINDS = ["normal", "greenish", "bluish"]


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


class Shared:
    """Oracle results that several tests need, computed once and never written to."""

    def __init__(self, orc):
        self.orc, self.kept = orc, {}

    def get(self, key, make):
        if key not in self.kept:
            v = make()
            for a in v if isinstance(v, tuple) else (v,):
                a.setflags(write=False)
            self.kept[key] = v
        return self.kept[key]

    def of_cube(self, name, fn):
        """fn(cube) for a per-pixel fn, (2^24, ...) rows in cube order."""
        return self.get(name, lambda: fn(K.cube()).reshape(K.N, -1))

    def before(self, key, u8):
        """strategy 2's image before CLAHE (parameters colour_cases.STRATEGY2) for a frame."""
        return self.get(("before", key), lambda: K.strategy2_before_clahe(self.orc, u8)[0])


@pytest.fixture(scope="module")
def shared(orc):
    return Shared(orc)


def frame_of(order):
    """(frame, row index into per-pixel results in cube order)."""
    if order == "cube":
        return K.cube(), slice(None)
    return K.shuffled()


def on_device(dev, array):
    return dev.tensor(np.array(array))  # the cached frames are read-only: torch wants its own writable copy


# ------------------------------------------------------------------------------------------------------ stage kernels
@pytest.mark.parametrize("order", ORDERS)
def test_rgb2lab_every_colour(dev, orc, shared, order):
    u8, rows = frame_of(order)
    want = shared.of_cube("lab", orc.cv_rgb2lab_u8)[rows].reshape(u8.shape)
    same(dev.rgb2lab_u8(on_device(dev, u8)).cpu().numpy(), want, f"rgb2lab_u8 on the {order}")


@pytest.mark.parametrize("order", ORDERS)
def test_lab2rgb_every_lab_byte_triple(dev, orc, shared, order):
    """The cube read as LAB bytes: out-of-gamut triples included, down to the negative and up to the far-cubic end of abToXZ."""
    lab, rows = frame_of(order)
    want = shared.of_cube("rgb", orc.cv_lab2rgb_u8)[rows].reshape(lab.shape)
    same(dev.lab2rgb_u8(on_device(dev, lab)).cpu().numpy(), want, f"lab2rgb_u8 on the {order}")


@pytest.mark.parametrize("shift", [14, 15])
@pytest.mark.parametrize("order", ORDERS)
def test_rgb2gray_every_colour(dev, orc, shared, order, shift):
    u8, rows = frame_of(order)
    want = shared.of_cube(("gray", shift), lambda c: orc.cv_rgb2gray_u8(c, shift))[rows].reshape(u8.shape[:2])
    same(dev.rgb2gray_u8(on_device(dev, u8), shift).cpu().numpy(), want, f"rgb2gray_u8 shift {shift} on the {order}")


@pytest.mark.parametrize("order", ORDERS)
def test_clahe_f32_on_the_float_cube(dev, orc, order):
    """uwie_clahe_f32 (k_quant_rgb2lab, k_lab2rgb_f32) on a float32 image that truncates to the cube's bytes."""
    img = K.perturbed_float(frame_of(order)[0], np.float32)
    same(dev.clahe_f32(dev.tensor(img[None]), 2.0, (8, 8))[0].cpu().numpy(), orc.SixStrategyOracle.clahe(img, 2.0, (8, 8)),
         f"clahe_f32 on the float {order}")


@pytest.mark.parametrize("order,dtype", [("cube", np.float32), ("shuffled", np.float64)])
def test_dict_general_float_route_on_the_float_cube(uw, dev, orc, order, dtype):
    """dict clahe_enhancement on a general float image (not u8 / 255 data: tests/test_colour_cases.py): the stage kernels
    behind uwie_enhance_f32 / _f64, the stretch after them on the reference's percentiles."""
    x = K.perturbed_float(frame_of(order)[0], dtype)
    params = dict(clip_limit=2.0, tile_grid_size=(8, 8), apply_gamma=False)
    want = orc.DictStrategyOracle.run(x, "clahe_enhancement", params)
    out, outf = dev.enhance_float(dev.tensor(x[None]), uw.api._dict_params(dev, "clahe_enhancement", params))
    tag = f"dict clahe_enhancement on the general {dtype.__name__} {order}"
    same(outf[0].cpu().numpy(), want, tag)
    same(out[0].cpu().numpy(), (want * 255).astype(np.uint8), tag + " bytes")


# ------------------------------------------------------------------------------------- to_lab of the code domain (<2>)
@pytest.mark.parametrize("order", ORDERS)
def test_code_domain_every_code_triple(uw, dev, orc, order):
    """k_stretch_lab_lut<2> with an identity code table: every byte triple through to_lab, raw codes and histogram through
    k_clahe_apply_codes, v -> max(v - 1, 0) behind it."""
    u8 = frame_of(order)[0]
    want8, want32, want64 = K.dict_clahe(orc, u8, 2.0, (8, 8))
    p = uw.api._dict_params(dev, "clahe_enhancement", dict(K.DICT_IDENTITY, clip_limit=2.0, tile_grid_size=(8, 8)))
    d_in = on_device(dev, u8[None])
    out, outf = dev.enhance_u8_f64(d_in, p)
    tag = f"dict clahe_enhancement, identity codes, on the {order}"
    same(out[0].cpu().numpy(), want8, tag + " bytes")
    same(outf[0].cpu().numpy(), want64, tag + " float64")
    out, outf = dev.enhance_u8(d_in, p, want_float=True)
    same(out[0].cpu().numpy(), want8, tag + " bytes beside the float32 image")
    same(outf[0].cpu().numpy(), want32, tag + " float32")


def test_strategy6_on_the_cube(dev, orc):
    """A stretch before CLAHE: a non-identity s_gcode table in front of to_lab, the final-table mode of k_clahe_apply_codes
    behind it.  pow: <= 1 LSB, 2e-7 on the float32 image."""
    u8 = K.cube()
    x = orc.normalise_u8(u8)
    assert orc.classify_cast(x) == "normal"
    wantf = orc.SixStrategyOracle.strategy(6, x)
    out, outf = dev.enhance_u8(on_device(dev, u8[None]), dev.params(0, 6), want_float=True)
    bytes_ok(out[0].cpu().numpy(), orc.quantise_u8(wantf), "strategy 6 on the cube", True)
    assert np.abs(outf[0].cpu().numpy().astype(np.float64) - wantf).max() <= 2e-7


# ------------------------------------------------------------- lab_of (<1>, both forms) and to_lab of stored planes (<0>)
def strategy2_params(dev, clip, tiles, **more):
    return dev.params(0, 2, clip_limit=clip, tiles_x=tiles[0], tiles_y=tiles[1], **K.STRATEGY2, **more)


def strategy2_on_device(dev, d_in, p, want8, wantf, tag):
    """Bytes alone (k_clahe_apply_u8) and bytes with the float image (k_clahe_apply_f32)."""
    out, _ = dev.enhance_u8(d_in, p)
    same(out[0].cpu().numpy(), want8, tag + " (k_clahe_apply_u8)")
    out, outf = dev.enhance_u8(d_in, p, want_float=True)
    same(out[0].cpu().numpy(), want8, tag + " (k_clahe_apply_f32)")
    same(outf[0].cpu().numpy(), wantf, tag + " float image")


@pytest.mark.parametrize("i", range(4))
def test_strategy2_quarter_through_every_source_form(dev, orc, shared, i):
    """A quarter's bytes are the codes (test_quarter_reaches_lab_with_its_own_bytes): the four quarters hand all 2^24 code
    triples to lab_of in the 1024-thread form (8 x 8 tiles) and in the fast path of the 256-thread form (32 x 32), and with
    stored planes to to_lab of <0>.  No pow: everything equal."""
    q = K.quarter(i)
    before = shared.before(i, q)
    d_in = on_device(dev, q[None])
    for tiles, _ in K.QUARTER_GRIDS:
        want8, wantf = K.strategy2(orc, before, 2.0, tiles)
        for store in (0, 1):
            with dev.tuning(restore_store=store):
                strategy2_on_device(dev, d_in, strategy2_params(dev, 2.0, tiles), want8, wantf,
                                    f"quarter {i} tiles {tiles} restore_store={store}")


def test_strategy2_quarter_takes_the_routes_it_is_aimed_at(dev):
    """As test_routes of tests/test_gpu_clahe_tail.py: the plan's wide_lut on each side, and the kernels the profiler saw."""
    from underwater_image_enhancement_amd import _lib

    d_in = on_device(dev, K.quarter(0)[None])
    dev.profile(True)
    try:
        for tiles, wide in K.QUARTER_GRIDS:
            assert _lib.clahe_plan(1, K.QUARTER, K.QUARTER, tiles, 2.0, recomputed=True).wide_lut == wide
            assert _lib.clahe_plan(1, K.QUARTER, K.QUARTER, tiles, 2.0, recomputed=False).wide_lut == 0
            for want_float in (False, True):
                apply_row = ["k_clahe_apply_f32" if want_float else "k_clahe_apply_u8"]
                dev.profile_rows()
                dev.enhance_u8(d_in, strategy2_params(dev, 2.0, tiles), want_float=want_float)
                assert lut_and_apply_rows(dev) == (["k_stretch_lab_lut_wide" if wide else "k_stretch_lab_lut<1>"], apply_row), tiles
                with dev.tuning(restore_store=1):
                    dev.enhance_u8(d_in, strategy2_params(dev, 2.0, tiles), want_float=want_float)
                    assert lut_and_apply_rows(dev) == (["k_stretch_lab_lut<0>"], apply_row), tiles
    finally:
        dev.profile(False)


def test_strategy2_quarter_under_f32t_is_identical(dev, orc, shared):
    """inter_dtype = F32T keeps the transmission in float32.  Here t is 1 everywhere, which float32 holds exactly, so the
    restore's quotient is the float64 route's and the result has to be identical, not merely within F32T's stated tolerance."""
    from underwater_image_enhancement_amd import _lib

    q = K.quarter(1)
    d_in = on_device(dev, q[None])
    for tiles, _ in K.QUARTER_GRIDS:
        want8, wantf = K.strategy2(orc, shared.before(1, q), 2.0, tiles)
        strategy2_on_device(dev, d_in, strategy2_params(dev, 2.0, tiles, inter_dtype=_lib.INTER_F32T), want8, wantf,
                            f"quarter 1 tiles {tiles} inter_dtype=F32T")


# --------------------------------------------------------------------------- the inline LAB2RGB of k_clahe_apply_out
@pytest.mark.parametrize("case", K.LAB_FRAMES, ids=[c.id for c in K.LAB_FRAMES])
def test_lab2rgb_inside_the_blend_kernel(uw, dev, orc, shared, case):
    """The (L', a, b) of test_lab_frames_reach_the_blend_kernels_domain through k_clahe_apply_u8 (one composed table),
    _f32 (two-step lookup) and _codes (raw codes and histogram)."""
    u8 = K.lab_frame(orc, case)
    d_in = on_device(dev, u8[None])
    want8, wantf = K.strategy2(orc, shared.before(case.name, u8), case.clip, case.tiles)
    strategy2_on_device(dev, d_in, strategy2_params(dev, case.clip, case.tiles), want8, wantf, f"{case.id} strategy 2")
    want8, want32, want64 = K.dict_clahe(orc, u8, case.clip, case.tiles)
    p = uw.api._dict_params(dev, "clahe_enhancement", dict(K.DICT_IDENTITY, clip_limit=case.clip, tile_grid_size=case.tiles))
    out, outf = dev.enhance_u8_f64(d_in, p)
    same(out[0].cpu().numpy(), want8, f"{case.id} dict clahe_enhancement bytes")
    same(outf[0].cpu().numpy(), want64, f"{case.id} dict clahe_enhancement float64")
    same(dev.enhance_u8(d_in, p, want_float=True)[1][0].cpu().numpy(), want32, f"{case.id} dict clahe_enhancement float32")


# ------------------------------------------------------------------------------------------------------- gray planes
@pytest.mark.parametrize("kind", CAST_KINDS)
def test_gray_planes_of_the_cast_corrected_cube(dev, orc, kind):
    """The 8-bit gray of the cast-corrected frame as k_quant_gray (transmission_init) and the quadtree (atmospheric_light:
    its own k_quant_gray with entry_fuse 0, the Canny pre-pass k_gray_strong with 1 and 2) write it, every colour, both shifts.
    (The plane cast detection's chunk pass writes for a guessed kind exists inside uwie_enhance_u8 only.)"""
    u8 = K.shuffled()[0] if kind == "greenish" else K.cube()
    frames = on_device(dev, u8[None])
    kk = dev.tensor(np.array([CAST_KINDS.index(kind)], np.int32))
    corrected = (orc.correct_cast(orc.normalise_u8(u8), kind) * 255).astype(np.uint8)
    A = dev.tensor(np.full((1, 3), 0.8, np.float32))
    for shift in (14, 15):
        want = orc.cv_rgb2gray_u8(corrected, shift)
        p = dev.params(0, 2, gray_shift=shift)
        same(dev.transmission_init(frames, A, kk, p)[1][0].cpu().numpy(), want, f"{kind} shift {shift} transmission_init")
        for fuse in (0, 1, 2):
            with dev.tuning(entry_fuse=fuse):
                _, gray = dev.atmospheric_light(frames, kk, p, want_gray=True)
                dev.check_status()
            same(gray[0].cpu().numpy(), want, f"{kind} shift {shift} atmospheric_light entry_fuse={fuse}")
