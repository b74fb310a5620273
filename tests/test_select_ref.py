"""CPU checks of tests/select_ref.py, the reference the selection tests (test_gpu_select.py) demand bit for bit."""
import numpy as np
import pytest

import select_ref as sr

QS = (0, 1e-7, 2.5, 15, 50, 97.5, 99.999, 100)


def test_known_answers_on_hand_made_planes():
    # n = 1: every percentile is the one value, both neighbours position 0
    for dt in (np.float32, np.float64):
        one = np.full((1, 1, 1, 3), 0.25, dt)
        for q in QS:
            assert sr.percentile_indices(1, q, dt)[:2] == (0, 0)
        assert (sr.percentiles(one, QS) == dt(0.25)).all()
        assert (sr.order_stats(one, QS) == dt(0.25)).all()
    # five values: (n - 1) * q integral at q = 0, 25, 50, 75, 100 -> gamma 0, the value at that position
    x = np.array([3.0, -1.0, 7.0, 2.0, 5.0], np.float32)
    img = np.repeat(x.reshape(1, 1, 5, 1), 3, axis=3)
    s = np.sort(x)
    for q, k in ((0, 0), (25, 1), (50, 2), (75, 3)):
        prev, nxt, t = sr.percentile_indices(5, q, np.float32)
        assert (prev, nxt, t) == (k, k + 1, 0)
        assert sr.percentiles(img, [q])[0, 0, 0] == s[k]
        assert tuple(sr.order_stats(img, [q])[0, 0, 0]) == (s[k], s[k + 1])
    assert sr.percentile_indices(5, 100, np.float32) == (4, 4, 0)  # above bounds: both the maximum
    assert tuple(sr.order_stats(img, [100])[0, 1, 0]) == (7.0, 7.0)
    # ties at the rank: the order statistic is the tied value whatever the neighbours
    t = np.array([0.5] * 6 + [0.25, 0.75], np.float64).reshape(1, 1, 8, 1).repeat(3, axis=3)
    assert (sr.order_stats(t, [50]) == 0.5).all()
    assert (sr.percentiles(t, [50]) == 0.5).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_against_sort_and_numpy(dtype):
    rng = np.random.default_rng(7)
    for shape in ((1, 1, 2, 3), (2, 7, 9, 3), (1, 83, 129, 3), (3, 1, 5, 3)):
        img = rng.normal(0, 1, shape).astype(dtype)
        img.reshape(-1)[:: 5] = img.reshape(-1)[0]  # ties
        p = sr.planes(img)
        n = p.shape[2]
        os_ = sr.order_stats(img, QS)
        pct = sr.percentiles(img, QS)
        assert pct.dtype == dtype and os_.dtype == dtype
        for b in range(p.shape[0]):
            for c in range(3):
                s = np.sort(p[b, c])
                for j, q in enumerate(QS):
                    prev, nxt, g = sr.percentile_indices(n, q, dtype)
                    assert os_[b, c, j, 0] == s[prev] and os_[b, c, j, 1] == s[nxt]
                    want = np.percentile(p[b, c], q)
                    assert np.asarray(want).dtype == dtype
                    assert sr.lerp(s[prev], s[nxt], g) == want
                    assert pct[b, c, j] == want


def test_index_arithmetic_past_2_24_follows_numpy():
    """Beyond 2^24 values float32 cannot hold every position: NumPy rounds (n - 1) * q in float32, so the position can
    differ from the float64 one.  np.percentile itself is the arbiter (a plane whose value is its position)."""
    seen_float32_rounding = False
    for n in (2**24 + 1, 2**24 + 3):
        plane = np.arange(n, dtype=np.float32)  # exact up to 2^24; beyond, value(k) rounds to even like position k
        idx64 = np.arange(n, dtype=np.float64)
        for q in (1e-7, 2.5, 15, 33.3, 50, 85, 97.5, 99.999):
            prev, nxt, g = sr.percentile_indices(n, q, np.float32)
            want = np.percentile(plane, q)
            assert sr.lerp(plane[prev], plane[nxt], g) == want, (n, q)
            # the positions: NumPy's float64 arithmetic on a float64 index plane reveals float32 vs float64 rounding
            p64 = sr.percentile_indices(n, q, np.float64)[0]
            seen_float32_rounding |= prev != p64
            assert 0 <= prev <= nxt <= n - 1
        assert sr.percentile_indices(n, 100, np.float32)[:2] == (n - 1, n - 1)
        assert np.percentile(idx64, 50) == sr.lerp(idx64[sr.percentile_indices(n, 50, np.float64)[0]],
                                                   idx64[sr.percentile_indices(n, 50, np.float64)[1]],
                                                   sr.percentile_indices(n, 50, np.float64)[2])
    assert seen_float32_rounding  # the case the float32 arithmetic exists for
    # the issue's example: 4100 x 4100 at q = 2.5 -- rank 420250 in float32, 420249 in float64
    assert sr.percentile_indices(4100 * 4100, 2.5, np.float32)[0] == 420250
    assert sr.percentile_indices(4100 * 4100, 2.5, np.float64)[0] == 420249


def test_chain_from_order_stats_is_the_oracles_chain():
    """k_pct_finish_chain applies f1 to the order statistics (f1 monotone): the same as the white balance's percentiles
    of f1(img), including the ties clip makes at 0 and 1."""
    rng = np.random.default_rng(11)
    cases = [rng.random((2, 37, 53, 3), np.float32),
             np.clip(rng.normal(0.5, 0.4, (1, 64, 48, 3)), 0, 1).astype(np.float32),  # many values clip to 0 / 1
             np.repeat(np.linspace(0, 1, 9, dtype=np.float32), 3).reshape(1, 1, 9, 3),
             np.full((1, 5, 5, 3), 0.5, np.float32)]
    for img in cases:
        for (lo, hi, wb) in ((20, 85, 2), (5, 98, 2), (40, 60, 10), (0, 100, 0)):
            want = sr.chain_percentiles(img, lo, hi, wb)
            got = sr.chain_from_order_stats(img, lo, hi, wb)
            sr.assert_same(got, want, f"{img.shape} {(lo, hi, wb)}")


def test_positions_of_the_differentiable_modules():
    n = 12
    assert list(sr.stretch_positions(np.float32([0, 100, 50, -5, 250]), n)) == [0, 11, 6, 0, 11]
    assert list(sr.gated_positions(np.float32([0, 50, 99]), n)) == [0, 6, 11]
    with pytest.raises(IndexError):
        sr.gated_positions(np.float32([100]), n)
    # L / 100.0 * n lands on an integer in float64 (25 % of 12 = 3); one float32 ulp below it truncates to 2
    assert sr.stretch_positions(np.float32([25]), n)[0] == 3
    assert sr.stretch_positions(np.nextafter(np.float32(25), np.float32(0)).reshape(1), n)[0] == 2


def test_same_bits_sees_signed_zero():
    a = np.array([0.0, 1.0, np.nan], np.float32)
    b = np.array([-0.0, 1.0, np.nan], np.float32)
    assert list(sr.same_bits(a, b)) == [False, True, True]
    with pytest.raises(AssertionError, match=r"-0.0 vs \+0.0"):
        sr.assert_same(a, b, "zeros")
