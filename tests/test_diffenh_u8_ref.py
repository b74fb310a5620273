"""The byte route (tests/diffenh_u8_ref.py) against the module's own route, torch.sort of the float image
(oracle.diff_enhance): the same float32 image bit for bit and the bytes of process_single_image's quantisation, on every
case of tests/diffenh_u8_cases.py.  Pins the monotonicity and rank argument of DESIGN.md section 16 without a GPU."""
import numpy as np
import pytest

import diffenh_u8_cases as C
import diffenh_u8_ref as R
from oracle import uwie_oracle as orc

F32 = np.float32


def oracle_float(u8, cols, flags):
    """oracle.diff_enhance of u8 / 255, as [B,H,W,3]"""
    x = u8.astype(F32) / F32(255.0)
    cols = cols.copy()
    par = {"L_low": cols[:, 0:1], "L_high": cols[:, 1:2]}
    if flags & 1:
        par["omega"] = cols[:, 2:3]
    if flags & 2:
        par["gamma"] = cols[:, 3:4]
    out = orc.diff_enhance(np.ascontiguousarray(x.transpose(0, 3, 1, 2)), par)
    return np.ascontiguousarray(out.transpose(0, 2, 3, 1))


def test_case_preconditions():
    assert int(float(F32(29)) / 100.0 * 100) == 28 and int(float(F32(57)) / 100.0 * 100) == 56
    assert R.stretch_rank(29.0, 100) == 28 and R.stretch_rank(57.0, 100) == 56
    assert R.stretch_rank(0.0, 100) == 0 and R.stretch_rank(100.0, 100) == 99
    assert R.stretch_rank(-5.0, 100) == 0 and R.stretch_rank(150.0, 100) == 99 and R.stretch_rank(np.nan, 100) == 0
    assert R.stretch_rank(50.0, 1) == 0
    # k zeros then 255s: sorted position `rank` is the first 255 when k = rank, the last zero when k = rank + 1
    a, b = C.case("rank_k_eq_rank"), C.case("rank_k_eq_rank_plus_1")
    assert np.array_equal(R.order_statistics(a["u8"], a["cols"])[0], [[1, 1], [0, 1], [0, 0]])
    assert np.array_equal(R.order_statistics(b["u8"], b["cols"])[0], [[0, 1], [0, 0], [1, 1]])
    # the bases of the second and third 5x3 frames are not 16-byte multiples; the constant frame fills one bin per channel
    assert (5 * 3 * 3) % 16 != 0 and (2 * 5 * 3 * 3) % 16 != 0
    const = C.case("constant_1080p")["u8"]
    assert np.bincount(const[0, :, :, 1].ravel(), minlength=256)[200] == 1080 * 1920 > 65535
    # crossed ranks give a negative range, a constant frame 1e-8
    os_ = R.order_statistics(C.case("rank_low_above_high")["u8"], C.case("rank_low_above_high")["cols"])
    assert np.all(os_[0, :, 1] < os_[0, :, 0])
    os_ = R.order_statistics(C.case("rank_low_above_high_constant")["u8"], C.case("rank_low_above_high_constant")["cols"])
    assert np.all(os_[0, :, 1] == os_[0, :, 0])


def test_v_over_255_is_strictly_increasing():
    t = np.arange(256, dtype=F32) / F32(255.0)
    assert np.all(np.diff(t) > 0)


@pytest.mark.parametrize("name", C.names())
def test_byte_route_equals_the_sort_route(name):
    c = C.case(name)
    flag_sets = (0, 1, 2, 3) if c["u8"].size < 10 ** 6 else (3,)
    for flags in flag_sets:
        want = oracle_float(c["u8"], c["cols"], flags)
        got = R.float_image(c["u8"], c["cols"], flags)
        assert R.same_bits(got, want), (name, flags)
        with np.errstate(invalid="ignore"):
            want_u8 = (np.clip(want, 0, 1) * 255).astype(np.uint8)
        # NaN (non-finite parameters only) has no defined uint8 cast: the byte route defines it as 0
        want_u8[np.isnan(want)] = 0
        assert np.array_equal(R.quantise(got), want_u8), (name, flags)
        if c["finite"]:
            assert not np.isnan(want).any()
