"""Generate tests/golden/refloss.npz: ReferenceLoss on the REAL enhancement modules under CPU autograd.

TEST INFRASTRUCTURE, run by hand where the reference project is importable (its location: oracle/gen_golden.py's REF).
The modules are imported with oracle/gen_golden.py's inert stand-ins for the libraries they do not use here, as in
tests/gen_golden_dlp_grads.py.  Each case runs one of the two modules on seeded inputs, then the loss of
EndToEndTrainer (deep_learning_parameters.ReferenceLoss, the gated module) or CombinedLoss's L1 and MSE terms
(vgg_16_UIE.py:272-303 without the perceptual term, the vgg module), and backward() from the total.  Stored per case:
the inputs, the weights, l1, l2, total, dL/d(out) (the module's effective grad_out), the parameter gradients and
grad_img_stable (the module's grad_img with the order statistics' terms moved to the stable-sort rule's elements,
DESIGN.md sections 8 and 10).

Run:  python tests/gen_golden_refloss.py   (torch CPU, float32)
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)
import diffenh_grad_ref as RV  # noqa: E402
import dlp_grad_ref as RG  # noqa: E402
import gen_golden as gg  # noqa: E402

OUT = os.path.join(HERE, "golden", "refloss.npz")
GATED_KEYS = ("L_low", "L_high", "use_gamma", "gamma")


def cases(rng):
    """tag -> (module 'gated' / 'vgg', img, params dict of (B, 1) float32, weights, reference rule)."""
    f = np.float32

    def lh(B):
        return {"L_low": rng.uniform(1, 30, (B, 1)).astype(f), "L_high": rng.uniform(65, 99, (B, 1)).astype(f)}

    def gate(B, u=None):
        return {"use_gamma": rng.uniform(0, 1, (B, 1)).astype(f) if u is None else np.asarray(u, f).reshape(B, 1),
                "gamma": rng.uniform(0.5, 3.0, (B, 1)).astype(f)}

    u8 = lambda shape: f(rng.integers(0, 16, shape) * 17) / f(255.0)  # noqa: E731  16 grey levels: ties in every plane
    rnd = lambda shape: rng.random(shape, dtype=f)  # noqa: E731
    out = {}
    out["gated_u8ties_2x3x24x31"] = ("gated", u8((2, 3, 24, 31)), {**lh(2), **gate(2)}, (0.5, 0.5), "rand")
    out["gated_use0_2x3x13x19"] = ("gated", rnd((2, 3, 13, 19)), {**lh(2), **gate(2, [0.0, 0.0])}, (0.5, 0.5), "rand")
    out["gated_use1_2x3x11x23"] = ("gated", rnd((2, 3, 11, 23)), {**lh(2), **gate(2, [1.0, 1.0])}, (0.3, 0.5), "rand")
    out["gated_usemix_4x3x10x9"] = ("gated", rnd((4, 3, 10, 9)), {**lh(4), **gate(4, [0.0, 1.0, 0.37, 0.81])}, (0.5, 0.5),
                                    "rand")
    out["gated_equal_2x3x12x15"] = ("gated", u8((2, 3, 12, 15)), {**lh(2), **gate(2, [0.0, 0.0])}, (0.3, 0.5), "equal")
    out["gated_nanref_2x3x9x14"] = ("gated", rnd((2, 3, 9, 14)), {**lh(2), **gate(2)}, (0.5, 0.5), "nan")
    vg = lambda B: {"omega": rng.uniform(0.3, 0.95, (B, 1)).astype(f), "gamma": rng.uniform(0.5, 2.5, (B, 1)).astype(f)}  # noqa: E731
    p = vg(2)
    out["vgg_u8ties_2x3x20x27"] = ("vgg", u8((2, 3, 20, 27)), {**lh(2), **p}, (0.3, 0.5), "rand")
    p = vg(2)
    out["vgg_omega_equal_2x3x14x17"] = ("vgg", rnd((2, 3, 14, 17)), {**lh(2), "omega": p["omega"]}, (0.5, 0.5), "equal")
    p = vg(3)
    out["vgg_gamma_3x3x9x21"] = ("vgg", rnd((3, 3, 9, 21)), {**lh(3), "gamma": p["gamma"]}, (0.3, 0.5), "rand")
    out["vgg_stretch_1x3x16x16"] = ("vgg", u8((1, 3, 16, 16)), lh(1), (0.5, 0.5), "rand")
    return out


def main():
    for name in ("torchvision", "torchvision.models", "torchvision.transforms"):
        mod = gg._Inert(name)
        mod.__path__ = []
        sys.modules.setdefault(name, mod)
    gg.import_reference()
    sys.path.insert(0, gg.REF)
    import torch
    import deep_learning_parameters as D
    import vgg_16_UIE as V

    rng = np.random.default_rng(20261017)
    out = {}
    for tag, (kind, img, par, (w1, w2), rule) in cases(rng).items():
        B = img.shape[0]
        enh = D.DifferentiableEnhancement() if kind == "gated" else V.DifferentiableEnhancement()
        with torch.no_grad():
            o0 = enh(torch.from_numpy(img), {k: torch.from_numpy(v) for k, v in par.items()}).numpy()
        ref = rng.random(img.shape, dtype=np.float32)
        if rule == "equal":  # o == r on about a third of the values: sgn(0) = 0.  Only where the forward is exact (no pow):
            # a 1-ulp pow difference would turn sgn(0) into +-1 there
            m = rng.random(img.shape) < 0.35
            ref[m] = o0[m]
        elif rule == "nan":
            ref[1, 2, 3, 4] = np.nan
        x = torch.from_numpy(img.copy()).requires_grad_(True)
        leaves = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in par.items()}
        res = enh(x, leaves)
        res.retain_grad()
        r = torch.from_numpy(ref)
        if kind == "gated":
            loss, parts = D.ReferenceLoss(l1_weight=w1, l2_weight=w2)(res, r)
            l1, l2 = parts["l1"], parts["l2"]
        else:  # CombinedLoss's L1 and MSE terms
            l1t, l2t = torch.nn.L1Loss()(res, r), torch.nn.MSELoss()(res, r)
            loss = w1 * l1t + w2 * l2t
            l1, l2 = l1t.item(), l2t.item()
        loss.backward()
        assert leaves["L_low"].grad is None and leaves["L_high"].grad is None, tag
        assert np.array_equal(res.detach().numpy(), o0, equal_nan=True), tag
        g = res.grad.numpy()
        gimg = x.grad.numpy()
        # the stable-sort rule's elements (tests/gen_golden_dlp_grads.py)
        xd = torch.from_numpy(img).requires_grad_(True)
        if kind == "gated":
            RG.gated(xd, *(torch.from_numpy(par[k]) for k in GATED_KEYS), detach_stats=True).backward(torch.from_numpy(g))
        else:
            tp = lambda k: torch.from_numpy(par[k]) if k in par else None  # noqa: E731
            RV.diff_enhance(xd, tp("L_low"), tp("L_high"), tp("omega"), tp("gamma"), detach_stats=True).backward(torch.from_numpy(g))
        per_px = xd.grad.numpy()
        n = img.shape[2] * img.shape[3]
        R = RG if kind == "gated" else RV
        klo, khi = R.sorted_positions(par["L_low"], n), R.sorted_positions(par["L_high"], n)
        stable = gimg.copy()
        for b in range(B):
            for c in range(3):
                flat = torch.from_numpy(img[b, c].reshape(-1))
                tq = [int(torch.sort(flat).indices[int(k)]) for k in (klo[b], khi[b])]
                sq = [R.stable_sort_source(img[b, c], int(k)) for k in (klo[b], khi[b])]
                d, mm, o = per_px[b, c].reshape(-1), gimg[b, c].reshape(-1), stable[b, c].reshape(-1)
                same = (d == mm) | (np.isnan(d) & np.isnan(mm))
                moved = set(np.flatnonzero(~same).tolist())
                assert moved <= set(tq), f"{tag} image {b} channel {c}: gradient at {sorted(moved)}, torch's sort says {tq}"
                o[:] = d
                if klo[b] == khi[b]:
                    o[sq[0]] = d[sq[0]] + (mm[tq[0]] - d[tq[0]])
                else:
                    for a, s in zip(tq, sq):
                        o[s] = d[s] + (mm[a] - d[a])
        rec = {"kind": np.array(0 if kind == "gated" else 1), "img": img, "ref": ref, "w": np.array([w1, w2], np.float32),
               "l1": np.float32(l1), "l2": np.float32(l2), "total": loss.detach().numpy(), "grad_out": g,
               "grad_img_stable": stable}
        for k, v in par.items():
            rec[k] = v
            if leaves[k].grad is not None:
                rec["grad_" + k] = leaves[k].grad.numpy()
        for k, v in rec.items():
            out[f"{tag}/{k}"] = v
        print(f"{tag}: l1 {l1:.6g} l2 {l2:.6g} total {loss.item():.6g}")
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
