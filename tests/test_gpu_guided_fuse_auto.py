"""The fused transmission route of the guided filter (k_guided_split8: t0 from the frame's bytes, no k_trans_init, no t0 plane)
and the size rule that makes it the default route of chip-filling jobs (tuning gf_fuse = 2, plan_guided).

The kernel runs four strips to a workgroup around one 3 KB table of the image's quotients, workgroups folded over the XCDs.
The forced cases (gf_fuse = 1, gf_bands = 2) are the smallest shapes at which that launch shape can go wrong:
  (3, 96, 232)   three strips x two bands = six items per image: the last workgroup has two idle wavefronts behind the barrier;
                 both strips at the image's edges and one interior strip
  (1, 200, 256)  a single image
  (5, 64, 1000)  ten strips x two bands in five images: 25 workgroups, a remainder of one over the eight XCDs; three cast kinds,
                 so a workgroup that took another image's table would show
Bytes: strategy 2 equals the oracle byte for byte (what test_enhance_matches_oracle asks of it), dict strong_dehazing within
1 LSB (what the dict-surface tests ask of a gamma strategy), and both are IDENTICAL to the unfused route (gf_fuse = 0).

The auto rule: strips x bands x B (uwie_guided_fill) against kFuseRounds = 1 round of the device's compute units x 8.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FUSE_ROUNDS = 1  # kFuseRounds (k_guided_pipe.hip; profiles/r05_fuse_route_sweep.txt)
SHAPES = [(3, 96, 232), (1, 200, 256), (5, 64, 1000)]
GAINS = [(0.45, 0.85, 0.80), (0.40, 0.70, 0.90), (0.80, 0.75, 0.70)]  # greenish, bluish, normal


@pytest.fixture(scope="module")
def dev():
    import underwater_image_enhancement_amd as uw

    d = uw.get_device()
    d.profile(True)
    yield d
    d.profile(False)


@pytest.fixture(scope="module")
def orc():
    from oracle import uwie_oracle

    return uwie_oracle


@pytest.fixture(scope="module")
def cases(orc):
    """{shape: (frames u8 [B,H,W,3], strategy-2 oracle bytes, strong_dehazing oracle bytes)}, computed once."""
    from test_gpu_configs import underwater

    out = {}
    for shape in SHAPES:
        B, H, W = shape
        rng = np.random.default_rng(B * 1000 + W)
        frames = np.stack([underwater(rng, H, W, GAINS[b % 3], noise=0.03) for b in range(B)])
        want2 = np.stack([orc.enhance_u8(f, 2) for f in frames])
        params = orc.CONFIG_STRATEGIES["strong_dehazing"]
        wantd = np.stack([(orc.DictStrategyOracle.run(orc.normalise_u8(f), "strong_dehazing", params) * 255).astype(np.uint8)
                          for f in frames])
        out[shape] = (frames, want2, wantd)
    return out


def guided_rows(dev):
    rows = dev.profile_rows()
    return {n: c for n, (_, c) in rows.items() if n.startswith("k_guided") or n == "k_trans_init"}


def run(dev, frames, p, fuse, bands=0):
    """(bytes, guided-filter profiler rows) of one enhance_u8 call under tuning gf_fuse = fuse (None: the default tuning)."""
    tune = {} if fuse is None else {"gf_fuse": fuse}
    if bands:
        tune["gf_bands"] = bands
    dev.profile_rows()
    with dev.tuning(**tune):
        out, _ = dev.enhance_u8(frames, p)
        rows = guided_rows(dev)
    return out, rows


def test_cast_kinds_of_the_batched_case(orc, cases):
    kinds = [orc.classify_cast(orc.normalise_u8(f)) for f in cases[(5, 64, 1000)][0]]
    assert set(kinds) == {"greenish", "bluish", "normal"}, kinds


@pytest.mark.parametrize("shape", SHAPES)
def test_fused_kernel_against_the_oracle_and_the_unfused_route(dev, cases, shape):
    from underwater_image_enhancement_amd import _lib

    frames, want2, wantd = cases[shape]
    x = dev.tensor(frames)
    p2 = dev.params(_lib.SURFACE_SIX, 2)
    pd = dev.params(_lib.SURFACE_DICT, _lib.DICT_STRATEGIES["strong_dehazing"], apply_gamma=1, gamma=1.2)
    for what, p, want, lsb in (("strategy 2", p2, want2, 0), ("strong_dehazing", pd, wantd, 1)):
        fused, rows = run(dev, x, p, 1, bands=2)
        assert rows == {"k_guided_split8": 1}, (what, rows)
        plain, rows0 = run(dev, x, p, 0, bands=2)
        assert rows0 == {"k_guided_split": 1, "k_trans_init": 1}, (what, rows0)
        got = fused.cpu().numpy()
        d = np.abs(got.astype(int) - want.astype(int))
        print(f"{what} {shape}: max |delta| vs oracle {d.max()} LSB, {np.count_nonzero(d)} of {d.size} bytes differ")
        assert d.max() <= lsb, f"{what} {shape}: max |delta| = {d.max()} LSB, {np.count_nonzero(d > lsb)} bytes beyond {lsb}"
        assert np.array_equal(got, plain.cpu().numpy()), f"{what} {shape}: fused and unfused routes differ"


def test_fused_kernel_float32_transmission(dev, cases):
    from underwater_image_enhancement_amd import _lib

    x = dev.tensor(cases[(3, 96, 232)][0])
    p = dev.params(_lib.SURFACE_SIX, 2, inter_dtype=_lib.INTER_F32T)
    fused, rows = run(dev, x, p, 1, bands=2)
    assert rows == {"k_guided_split8": 1}, rows
    plain, rows0 = run(dev, x, p, 0, bands=2)
    assert rows0 == {"k_guided_split": 1, "k_trans_init": 1}, rows0
    assert np.array_equal(fused.cpu().numpy(), plain.cpu().numpy())


def fill(dev, B, H, W):
    """Strip-wavefronts of the default plan (0: no split plan)."""
    items, r0, rows = ctypes.c_longlong(), ctypes.c_int(), ctypes.c_int()
    from underwater_image_enhancement_amd import _lib

    _lib.check(dev.lib.uwie_guided_plan(B, H, W, 15, ctypes.byref(r0), ctypes.byref(rows)))
    _lib.check(dev.lib.uwie_guided_fill(B, H, W, 15, ctypes.byref(items)))
    assert (items.value > 0) == (rows.value > 0)
    return items.value


def test_auto_route_by_job_size(dev):
    """4K frames, the smallest batch that fills FUSE_ROUNDS rounds of the resident strip-wavefronts and the batch below it."""
    import torch

    from underwater_image_enhancement_amd import _lib

    H, W = 2160, 3840
    need = FUSE_ROUNDS * 8 * torch.cuda.get_device_properties(dev.torch_device).multi_processor_count
    above = next(B for B in range(1, 257) if fill(dev, B, H, W) >= need)
    below = above - 1
    assert 0 < fill(dev, below, H, W) < need, (below, fill(dev, below, H, W), need)  # a split plan, short of the fill
    p = dev.params(_lib.SURFACE_SIX, 2)
    g = torch.Generator(device=dev.torch_device).manual_seed(11)
    frames = torch.randint(0, 256, (above, H, W, 3), generator=g, device=dev.torch_device, dtype=torch.uint8)
    for B, want in ((above, {"k_guided_split8": 1}), (below, {"k_guided_split": 1, "k_trans_init": 1})):
        x = frames[:B].contiguous()
        auto, rows = run(dev, x, p, None)
        assert rows == want, (B, rows)
        plain, rows0 = run(dev, x, p, 0)
        assert rows0 == {"k_guided_split": 1, "k_trans_init": 1}, (B, rows0)
        assert torch.equal(auto, plain), f"batch {B}: the default route and gf_fuse = 0 differ"
