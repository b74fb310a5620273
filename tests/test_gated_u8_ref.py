"""tests/gated_u8_ref.py (the byte-domain restatement the GPU tests lean on) against the float-image restatement of the gated
module, tests/dlp_grad_ref.py: equal bit for bit where use_gamma = 0, within 1 float32 ulp otherwise (torch's vectorised
pow and its scalar tail differ in the last bit).  Also the preconditions of the rank cases."""
import numpy as np
import pytest
import torch

import dlp_grad_ref as D
import gated_u8_cases as C
import gated_u8_ref as R


def float_route(u8, cols):
    x = torch.from_numpy(u8.astype(np.float32) / np.float32(255.0))
    t = lambda i: torch.from_numpy(np.array(cols[:, i:i + 1]))  # noqa: E731
    with torch.no_grad():
        return D.gated(x, t(0), t(1), t(2), t(3), planar=False).numpy()


@pytest.mark.parametrize("name", C.names())
def test_equals_the_float_image_restatement(name):
    c = C.case(name)
    got, want = R.float_image(c["u8"], c["cols"]), float_route(c["u8"], c["cols"])
    assert np.all(got >= 0) and np.all(got <= 1)
    for b in range(c["u8"].shape[0]):
        if c["cols"][b, 2] == 0:
            assert R.same_bits(got[b], want[b]), (name, b)
        else:  # values in [0, 1]: the int32 words are ordered as the values
            ulp = np.abs(got[b].view(np.int32).astype(np.int64) - want[b].view(np.int32).astype(np.int64)).max()
            assert ulp <= 1, (name, b, ulp)
    assert np.array_equal(R.quantise(got), (np.clip(got, 0, 1) * 255).astype(np.uint8))
    # the order statistics are those of the float image
    x = c["u8"].astype(np.float32) / np.float32(255.0)
    n = x.shape[1] * x.shape[2]
    os_ = R.order_statistics(c["u8"], c["cols"])
    for b in range(x.shape[0]):
        for q in range(2):
            k = int(D.sorted_positions(c["cols"][b, q], n)[0])
            for ch in range(3):
                assert os_[b, ch, q] == np.sort(x[b, :, :, ch].reshape(-1))[k]


def test_rank_case_preconditions():
    n = C.N
    pos = lambda L: int(D.sorted_positions(np.float32(L), n)[0])  # noqa: E731
    assert pos(37.0) == 37
    eq, plus = C.case("rank_k_eq_rank"), C.case("rank_k_eq_rank_plus_1")
    for ch in range(3):
        assert np.sort(eq["u8"][0, :, :, ch].reshape(-1))[37] == 255 and np.sort(eq["u8"][0, :, :, ch].reshape(-1))[36] == 0
        assert np.sort(plus["u8"][0, :, :, ch].reshape(-1))[37] == 0 and np.sort(plus["u8"][0, :, :, ch].reshape(-1))[38] == 255
    assert np.array_equal(R.order_statistics(eq["u8"], eq["cols"])[:, 0], [[1.0, 1.0], [0.0, 1.0]])
    assert np.array_equal(R.order_statistics(plus["u8"], plus["cols"])[:, 0], [[0.0, 1.0], [0.0, 0.0]])
    # int() truncates toward zero, and a negative position counts from the end
    assert int(float(np.float32(-3.6)) / 100.0 * n) == -3 and pos(-3.6) == n - 3 and pos(-0.5) == 0
    neg = C.case("rank_negative")
    os_ = R.order_statistics(neg["u8"], neg["cols"])
    assert np.array_equal(os_[:, 0], [[1.0, 0.0], [0.0, 1.0], [0.0, 1.0]])  # 97 of 60 zeros: a 255; of 99 zeros: still a zero
    lh = C.case("rank_low_above_high")
    assert np.array_equal(R.order_statistics(lh["u8"], lh["cols"])[0, 0], [1.0, 0.0])
    same = C.case("rank_low_eq_high")
    os_ = R.order_statistics(same["u8"], same["cols"])
    assert np.array_equal(os_[:, :, 0], os_[:, :, 1])
    for L, exc in C.UNINDEXABLE:
        with pytest.raises(exc):
            D.sorted_positions(np.float32(L), n)
    assert [float(v) for v in C.case("use_gamma_0_1_037")["cols"][:, 2]] == [0.0, 1.0, float(np.float32(0.37))]
    assert [float(v) for v in C.case("gamma_1_15_05")["cols"][:, 3]] == [1.0, 1.5, 0.5]


def test_the_constant_frame_fills_one_bin():
    c = C.case("const_1x1080x1920")
    assert np.bincount(c["u8"][0, :, :, 0].reshape(-1), minlength=256)[131] == 2073600
    assert np.array_equal(R.order_statistics(c["u8"], c["cols"]), np.full((1, 3, 2), np.float32(131) / np.float32(255.0)))
