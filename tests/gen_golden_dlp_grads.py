"""Generate tests/golden/dlp_grads.npz: gradients of the REAL deep_learning_parameters.DifferentiableEnhancement (the
gated-gamma module EndToEndTrainer trains through) under CPU autograd.

TEST INFRASTRUCTURE, run by hand where the reference project is importable (its location: oracle/gen_golden.py's REF).
The module is imported with oracle/gen_golden.py's inert stand-ins for the libraries it does not use here; seeded inputs,
a seeded grad_out and the module's gradients are stored as small fixtures (only arrays travel).  As for
tests/gen_golden_vgg_grads.py, each case stores the module's own grad_img and grad_img_stable, the same gradient with the
order statistics' terms moved to the stable-sort rule's elements (DESIGN.md sections 8 and 10).  The "errors" group holds
L values the module cannot index and the exception each raised (0 IndexError, 1 ValueError, 2 OverflowError).

Run:  python tests/gen_golden_dlp_grads.py   (torch CPU, float32)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)
import dlp_grad_ref as R  # noqa: E402
import gen_golden as gg  # noqa: E402

OUT = os.path.join(HERE, "golden", "dlp_grads.npz")
ERRORS = (IndexError, ValueError, OverflowError)


def cases(rng):
    """tag -> (img, L_low, L_high, use_gamma, gamma)."""
    f = np.float32

    def lh(B, lo=(1, 30), hi=(65, 99)):
        return rng.uniform(*lo, (B, 1)).astype(f), rng.uniform(*hi, (B, 1)).astype(f)

    def ug(B, a=0.0, b=1.0):
        return rng.uniform(a, b, (B, 1)).astype(f)

    def ga(B, a=0.5, b=3.0):
        return rng.uniform(a, b, (B, 1)).astype(f)

    def full(B, v):
        return np.full((B, 1), v, f)

    out = {}
    # 16 grey levels: ties in every plane (stable-sort rule)
    img = f(rng.integers(0, 16, (2, 3, 24, 31)) * 17) / f(255.0)
    out["u8ties_2x3x24x31"] = (img, *lh(2), ug(2), ga(2))
    out["rand_3x3x17x40"] = (rng.random((3, 3, 17, 40), dtype=f), *lh(3), ug(3), ga(3))
    # flat planes: r = 1e-8
    out["flat_1x3x8x8"] = (np.full((1, 3, 8, 8), 0.5, f), *lh(1), ug(1), ga(1))
    # the gate at its ends and in between
    out["use0_2x3x13x19"] = (rng.random((2, 3, 13, 19), dtype=f), *lh(2), full(2, 0.0), ga(2))
    out["use1_2x3x11x23"] = (rng.random((2, 3, 11, 23), dtype=f), *lh(2), full(2, 1.0), ga(2))
    out["use037_2x3x12x15"] = (rng.random((2, 3, 12, 15), dtype=f), *lh(2), full(2, 0.37), ga(2))
    out["usemix_4x3x10x9"] = (rng.random((4, 3, 10, 9), dtype=f), *lh(4), np.array([[0.0], [1.0], [0.37], [0.81]], f), ga(4))
    # gamma inside the predictor's [1, 1.5] and outside it
    out["gammain_2x3x14x16"] = (rng.random((2, 3, 14, 16), dtype=f), *lh(2), ug(2), ga(2, 1.0, 1.5))
    out["gammaout_3x3x9x21"] = (rng.random((3, 3, 9, 21), dtype=f), *lh(3), ug(3), np.array([[0.5], [2.2], [3.0]], f))
    # L_low == L_high: both terms on one element (r = 1e-8 as well)
    img = f(rng.integers(0, 256, (2, 3, 9, 14))) / f(255.0)
    L = np.array([[40.0], [73.5]], f)
    out["sameL_2x3x9x14"] = (img, L, L.copy(), ug(2), ga(2))
    # n = 120: L_high = 99.5 -> int(119.4) = 119 = n - 1 exactly, L_low = 0
    out["khilast_1x3x10x12"] = (rng.random((1, 3, 10, 12), dtype=f), full(1, 0.0), full(1, 99.5), ug(1), ga(1))
    # negative L_low: int(-3.6) = -3 wraps to n - 3 (p_lo above p_hi); int(-0.6) = 0 (truncation toward zero)
    out["negL_2x3x10x12"] = (rng.random((2, 3, 10, 12), dtype=f), np.array([[-3.0], [-0.5]], f), full(2, 90.0), ug(2), ga(2))
    # ParameterPredictor's output ranges (deep_learning_parameters.py:150-153)
    out["predictor_3x3x32x32"] = (rng.random((3, 3, 32, 32), dtype=f), *lh(3, (5, 20), (85, 98)), ug(3), ga(3, 1.0, 1.5))
    # degenerate planes
    out["px_2x3x1x1"] = (rng.random((2, 3, 1, 1), dtype=f), *lh(2), ug(2), ga(2))
    out["row_1x3x1x37"] = (rng.random((1, 3, 1, 37), dtype=f), *lh(1), ug(1), ga(1))
    return out


def error_cases():
    """(L_low, L_high) per single image of 8x8 (n = 64) that the module cannot index."""
    return np.array([[100.0, 50.0], [50.0, 100.0], [-101.6, 50.0], [-105.0, 50.0], [np.nan, 50.0], [50.0, np.nan],
                     [np.inf, 50.0], [-np.inf, 50.0], [50.0, np.inf], [150.0, np.nan], [1e30, 50.0]], np.float32)


def main():
    gg.import_reference()
    sys.path.insert(0, gg.REF)
    import torch
    import deep_learning_parameters as D

    enh = D.DifferentiableEnhancement()
    rng = np.random.default_rng(20261016)
    out = {}
    for tag, (img, L_low, L_high, use_gamma, gamma) in cases(rng).items():
        B = img.shape[0]
        t = lambda a: torch.from_numpy(np.array(a)).requires_grad_(True)  # noqa: E731
        x, lo, hi, u, g_ = t(img), t(L_low), t(L_high), t(use_gamma), t(gamma)
        par = {"L_low": lo, "L_high": hi, "use_gamma": u, "gamma": g_}
        res = enh(x, par)
        g = rng.standard_normal(img.shape).astype(np.float32)
        res.backward(torch.from_numpy(g))
        assert lo.grad is None and hi.grad is None, tag
        gimg = x.grad.numpy()
        # where the order statistics' gradient went (see tests/gen_golden_vgg_grads.py)
        xd = torch.from_numpy(img).requires_grad_(True)
        dp = {k: v.detach() for k, v in par.items()}
        R.gated(xd, dp["L_low"], dp["L_high"], dp["use_gamma"], dp["gamma"], detach_stats=True).backward(torch.from_numpy(g))
        per_px = xd.grad.numpy()
        n = img.shape[2] * img.shape[3]
        klo, khi = R.sorted_positions(L_low, n), R.sorted_positions(L_high, n)
        stable = gimg.copy()
        src = np.zeros((B, 3, 4), np.int64)  # torch's lo, hi, the rule's lo, hi
        for b in range(B):
            for c in range(3):
                flat = torch.from_numpy(img[b, c].reshape(-1))
                tq = [int(torch.sort(flat).indices[int(k)]) for k in (klo[b], khi[b])]
                sq = [R.stable_sort_source(img[b, c], int(k)) for k in (klo[b], khi[b])]
                src[b, c] = tq + sq
                moved = set(np.flatnonzero(gimg[b, c].reshape(-1) != per_px[b, c].reshape(-1)).tolist())
                assert moved <= set(tq), f"{tag} image {b} channel {c}: gradient at {sorted(moved)}, torch's sort says {tq}"
                assert all(flat[a] == flat[s] for a, s in zip(tq, sq)), tag
                d, m, o = per_px[b, c].reshape(-1), gimg[b, c].reshape(-1), stable[b, c].reshape(-1)
                o[:] = d
                if klo[b] == khi[b]:
                    o[sq[0]] = d[sq[0]] + (m[tq[0]] - d[tq[0]])
                else:
                    for a, s in zip(tq, sq):
                        o[s] = d[s] + (m[a] - d[a])
        if not np.array_equal(src[:, :, :2], src[:, :, 2:]):
            print(f"{tag}: torch's default sort routes {np.count_nonzero(src[:, :, :2] != src[:, :, 2:])} of "
                  f"{src[:, :, :2].size} order-statistic gradients to another of the tied elements than a stable sort")
        for k, v in (("img", img), ("L_low", L_low), ("L_high", L_high), ("use_gamma", use_gamma), ("gamma", gamma),
                     ("grad_out", g), ("out", res.detach().numpy()), ("grad_img", gimg), ("grad_img_stable", stable),
                     ("src", src), ("grad_use_gamma", u.grad.numpy()), ("grad_gamma", g_.grad.numpy()),
                     ("k", np.stack([klo, khi], axis=1))):
            out[f"{tag}/{k}"] = v
        print(f"{tag}: |grad_img| max {np.abs(gimg).max():.4g}, grad_use_gamma {u.grad.numpy().ravel()}")
    # the exception the module raises for each unindexable pair
    Ls = error_cases()
    codes = []
    img = torch.from_numpy(rng.random((1, 3, 8, 8), dtype=np.float32))
    for lo, hi in Ls:
        par = {"L_low": torch.tensor([[lo]]), "L_high": torch.tensor([[hi]]), "use_gamma": torch.tensor([[0.5]]),
               "gamma": torch.tensor([[1.2]])}
        try:
            enh(img, par)
            raise AssertionError(f"({lo}, {hi}) did not raise")
        except ERRORS as e:
            codes.append(next(i for i, cls in enumerate(ERRORS) if type(e) is cls))
            print(f"errors: L = ({lo}, {hi}) -> {type(e).__name__}: {e}")
    out["errors/L"] = Ls
    out["errors/n"] = np.array(64)
    out["errors/code"] = np.array(codes, np.int64)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
