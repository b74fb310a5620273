"""Guided-filter kernel variants side by side: time per launch and max |t - t_ref| against the exact-order kernel.

usage: python profiles/gf_bench.py [H W B [k eps]]   (default 2160 3840 16 15 0.5)
       python profiles/gf_bench.py --sweep           (the fused transmission route against k_trans_init + k_guided_split by job size)
Variants are selected through the context's route selectors (uwie_set_tuning: gf_split) and the mode argument; the LDS-tiled
strip kernel (k_guided_fast) is timed on window 7, which the wavefront kernels do not take.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import underwater_image_enhancement_amd as uw  # noqa: E402



def sweep():
    """Tuning gf_fuse 1 against 0 on whole strategy-2 calls, 4K x {2 .. 64} and 1080p x {10, 64, 128}: where the fused route starts
    to win, in rounds of the chip's resident strip-wavefronts (compute units x 8) -- the evidence behind kFuseRounds
    (k_guided_pipe.hip).  Per job: the two settings alternate three times, each time REPS calls between two events."""
    import ctypes

    from underwater_image_enhancement_amd import _lib

    REPS = 5
    dev = uw.Device(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    p = dev.params(_lib.SURFACE_SIX, 2)
    print(f"# gf_fuse = 1 against 0, strategy 2, ms per call (min .. max of three alternating rounds of {REPS} calls); {cus} compute units,")
    print(f"# resident strip-wavefronts {cus * 8}; default: the route gf_fuse = 2 takes")
    print("# H W B items rounds | fuse=0 ms | fuse=1 ms | median diff ms | default route")
    jobs = [(2160, 3840, b) for b in (2, 4, 8, 16, 32, 64)] + [(1080, 1920, b) for b in (10, 64, 128)]
    for H, W, B in jobs:
        g = torch.Generator(device="cuda").manual_seed(B)
        frames = torch.randint(0, 256, (B, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
        items = ctypes.c_longlong()
        _lib.check(dev.lib.uwie_guided_fill(B, H, W, 15, ctypes.byref(items)))
        ms = {0: [], 1: []}
        for rnd in range(4):  # (round 0 warms up)
            for fuse in (0, 1):
                with dev.tuning(gf_fuse=fuse):
                    dev.enhance_u8(frames, p)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(REPS):
                        dev.enhance_u8(frames, p)
                    e1.record()
                    torch.cuda.synchronize()
                if rnd:
                    ms[fuse].append(e0.elapsed_time(e1) / REPS)
        dev.profile(True)
        dev.profile_rows()
        dev.enhance_u8(frames, p)
        rows = dev.profile_rows()
        dev.profile(False)
        route = "fused" if "k_guided_split8" in rows else "split" if "k_guided_split" in rows else "pipe"
        med = sorted(ms[1])[1] - sorted(ms[0])[1]
        print(f"{H} {W} {B:3d} {items.value:6d} {items.value / (cus * 8):5.2f} | {min(ms[0]):7.3f} .. {max(ms[0]):7.3f} | "
              f"{min(ms[1]):7.3f} .. {max(ms[1]):7.3f} | {med:+7.3f} | {route}", flush=True)
        del frames
        dev._workspace = None
        torch.cuda.empty_cache()


if len(sys.argv) > 1 and sys.argv[1] == "--sweep":
    sweep()
    sys.exit(0)

H, W, B = (int(v) for v in (sys.argv[1:4] if len(sys.argv) >= 4 else (2160, 3840, 16)))
k = int(sys.argv[4]) if len(sys.argv) > 4 else 15
eps = float(sys.argv[5]) if len(sys.argv) > 5 else 0.5
dev = uw.Device(0)
g = torch.Generator(device="cuda").manual_seed(1)
yy = torch.arange(H, device="cuda").view(1, H, 1)
xx = torch.arange(W, device="cuda").view(1, 1, W)
field = 0.5 + 0.25 * torch.sin(xx / 97.0) * torch.cos(yy / 61.0)
gray = (255 * (field + 0.03 * torch.randn((B, H, W), device="cuda", generator=g)).clamp(0, 1)).to(torch.uint8).contiguous()
t0 = (1.0 - 0.5 * (field * 0.9 + 0.05 * torch.rand((B, H, W), device="cuda", generator=g))).clamp(0.1, 1.0).float().contiguous()


def run(sel, exact=False, reps=5, kk=k):
    dev.tune(gf_split=1, gf_bands=0)
    dev.tune(**sel)
    t = dev.guided_filter(gray, t0, kk, eps, exact=exact)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        t = dev.guided_filter(gray, t0, kk, eps, exact=exact)
    e1.record()
    torch.cuda.synchronize()
    return t, e0.elapsed_time(e1) / reps


nb = min(B, 2)
refs = {}
for kk in (k, 7):
    ref, ms_ref = run({}, exact=True, reps=1, kk=kk)
    refs[kk] = ref[:nb].clone()
    print(f"{H}x{W} x{B} k={kk} eps={eps}")
    print(f"  exact-order kernels      {ms_ref:8.3f} ms")
for name, env, mode, kk in (("LDS-tiled strip kernel", {}, False, 7), ("pipe, f64 ring in LDS", {"gf_split": 0}, False, k),
                            ("pipe, f64 split ring", {}, False, k), ("pipe, fx32 ring", {}, 2, k)):
    t, ms = run(env, exact=mode, kk=kk)
    err = (t[:nb] - refs[kk]).abs().max().item()
    gbs = B * H * W * 13 / ms / 1e6
    print(f"  {name:24s} k={kk:2d} {ms:8.3f} ms   {gbs:7.1f} GB/s algorithmic   max|t - t_exact| = {err:.3e}")
