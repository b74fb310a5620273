"""Generate tests/golden/vgg_grads.npz: gradients of the REAL vgg_16_UIE.DifferentiableEnhancement under CPU autograd.

TEST INFRASTRUCTURE, run by hand where the reference project is importable (its location: oracle/gen_golden.py's REF).
The module is imported with oracle/gen_golden.py's inert stand-ins for the libraries it does not use here; seeded
inputs, a seeded grad_out and the module's gradients are stored as small fixtures (only arrays travel).  The generator
also checks where the gradient of each order statistic lands.  The contract is the stable-sort
rule (diffenh_grad_ref.stable_sort_source); torch's default CPU sort, which the module calls, is not stable for tied
values, so each case stores the module's own grad_img and grad_img_stable, the same gradient with the two scalar terms
moved to the rule's elements (src: torch's and the rule's element per plane).

Run:  python tests/gen_golden_vgg_grads.py   (torch CPU, float32)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)
import diffenh_grad_ref as R  # noqa: E402
import gen_golden as gg  # noqa: E402

OUT = os.path.join(HERE, "golden", "vgg_grads.npz")


def cases(rng):
    """tag -> (img, L_low, L_high, omega or None, gamma or None)."""
    def lh(B, lo=(1, 30), hi=(65, 99)):
        return rng.uniform(*lo, (B, 1)).astype(np.float32), rng.uniform(*hi, (B, 1)).astype(np.float32)

    def om(B, a=0.1, b=0.9):
        return rng.uniform(a, b, (B, 1)).astype(np.float32)

    def ga(B):
        return rng.uniform(0.5, 3.0, (B, 1)).astype(np.float32)

    out = {}
    # 16 grey levels: ties in every plane and between channels (stable-sort rule, first-min rule)
    img = np.float32(rng.integers(0, 16, (2, 3, 24, 31)) * 17) / np.float32(255.0)
    out["u8ties_2x3x24x31"] = (img, *lh(2), om(2), ga(2))
    img = rng.random((3, 3, 17, 40), dtype=np.float32)
    out["rand_3x3x17x40"] = (img, *lh(3), om(3), ga(3))
    # dark frame, strong omega: t = clamp(1 - omega * dark, 0.1, 1) and the recovery clamp both saturate
    img = rng.random((1, 3, 33, 21), dtype=np.float32) * np.float32(0.3)
    out["dark_1x3x33x21"] = (img, *lh(1), om(1, 0.92, 0.99), ga(1))
    # flat planes: r = 1e-8
    out["flat_1x3x8x8"] = (np.full((1, 3, 8, 8), 0.5, np.float32), *lh(1), om(1), ga(1))
    img = rng.random((2, 3, 16, 16), dtype=np.float32)
    out["stretch_2x3x16x16"] = (img, *lh(2), None, None)
    img = rng.random((2, 3, 13, 19), dtype=np.float32)
    out["omega_2x3x13x19"] = (img, *lh(2), om(2), None)
    img = rng.random((2, 3, 11, 23), dtype=np.float32)
    out["gamma_2x3x11x23"] = (img, *lh(2), None, ga(2))
    # L_low == L_high: both terms on one element (r = 1e-8 as well)
    img = np.float32(rng.integers(0, 256, (2, 3, 9, 14))) / np.float32(255.0)
    L = np.array([[40.0], [73.5]], np.float32)
    out["sameL_2x3x9x14"] = (img, L, L.copy(), om(2), ga(2))
    # L_low = 0, L_high = 100: the high index clamps to n - 1
    img = rng.random((1, 3, 10, 12), dtype=np.float32)
    out["ends_1x3x10x12"] = (img, np.zeros((1, 1), np.float32), np.full((1, 1), 100.0, np.float32), om(1), ga(1))
    # degenerate planes
    out["px_2x3x1x1"] = (rng.random((2, 3, 1, 1), dtype=np.float32), *lh(2), om(2), ga(2))
    out["row_1x3x1x37"] = (rng.random((1, 3, 1, 37), dtype=np.float32), *lh(1), om(1), ga(1))
    return out


def main():
    for name in ("torchvision", "torchvision.models", "torchvision.transforms"):
        mod = gg._Inert(name)
        mod.__path__ = []
        sys.modules.setdefault(name, mod)
    gg.import_reference()
    sys.path.insert(0, gg.REF)
    import torch
    import vgg_16_UIE as V

    enh = V.DifferentiableEnhancement()
    rng = np.random.default_rng(20261015)
    out = {}
    for tag, (img, L_low, L_high, omega, gamma) in cases(rng).items():
        B = img.shape[0]
        t = lambda a: torch.from_numpy(np.array(a)).requires_grad_(True)  # noqa: E731
        x, lo, hi = t(img), t(L_low), t(L_high)
        par = {"L_low": lo, "L_high": hi}
        if omega is not None:
            par["omega"] = t(omega)
        if gamma is not None:
            par["gamma"] = t(gamma)
        res = enh(x, par)
        g = rng.standard_normal(img.shape).astype(np.float32)
        res.backward(torch.from_numpy(g))
        assert lo.grad is None and hi.grad is None, tag
        gimg = x.grad.numpy()
        # Where the order statistics' gradient went.  torch's default CPU sort (the module's torch.sort(flat_channel)) is
        # NOT stable for tied values (torch 2.10): among the elements equal to p_lo / p_hi it may pick another one than
        # the stable-sort rule of the contract.  So: the module's gradient moved exactly at the elements its own sort
        # names; those hold the same value as the rule's elements; grad_img_stable is grad_img with the two terms moved
        # to the rule's elements (what the device computes; equal to grad_img wherever there is no tie).
        xd = torch.from_numpy(img).requires_grad_(True)
        dp = {k: v.detach() for k, v in par.items()}  # the parameters' .grad stays the module's
        R.diff_enhance(xd, dp["L_low"], dp["L_high"], dp.get("omega"), dp.get("gamma"), detach_stats=True).backward(
            torch.from_numpy(g))
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
                assert all(flat[t] == flat[u] for t, u in zip(tq, sq)), tag
                d, m, o = per_px[b, c].reshape(-1), gimg[b, c].reshape(-1), stable[b, c].reshape(-1)
                o[:] = d
                if klo[b] == khi[b]:
                    o[sq[0]] = d[sq[0]] + (m[tq[0]] - d[tq[0]])
                else:
                    for t, u in zip(tq, sq):
                        o[u] = d[u] + (m[t] - d[t])
        if not np.array_equal(src[:, :, :2], src[:, :, 2:]):
            print(f"{tag}: torch's default sort routes {np.count_nonzero(src[:, :, :2] != src[:, :, 2:])} of "
                  f"{src[:, :, :2].size} order-statistic gradients to another of the tied elements than a stable sort")
        out[f"{tag}/grad_img_stable"] = stable
        out[f"{tag}/src"] = src
        out[f"{tag}/img"] = img
        out[f"{tag}/L_low"] = L_low
        out[f"{tag}/L_high"] = L_high
        if omega is not None:
            out[f"{tag}/omega"] = omega
            out[f"{tag}/grad_omega"] = par["omega"].grad.numpy()
        if gamma is not None:
            out[f"{tag}/gamma"] = gamma
            out[f"{tag}/grad_gamma"] = par["gamma"].grad.numpy()
        out[f"{tag}/grad_out"] = g
        out[f"{tag}/out"] = res.detach().numpy()
        out[f"{tag}/grad_img"] = gimg
        out[f"{tag}/L_grad_is_none"] = np.array(lo.grad is None and hi.grad is None)
        print(f"{tag}: |grad_img| max {np.abs(gimg).max():.4g}")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
