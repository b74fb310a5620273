"""Which guided-filter kernels a call runs, read from the context's profiler: one table of cases over the strategies, the
dict dehazing sets, the float-image calls, uwie_guided_filter's modes and uwie_enhance_all_u8.

Routes (k_guided_pipe.hip, plan_guided):
  pipe   k_guided_pipe alone (windows 10 / 15 / 20, small jobs, odd widths, the fixed-point a/b ring)
  split  k_guided_split (window 15, even width, a large job or a forced band count)
  split+ k_guided_split and a k_guided_pipe border launch (windows 10 / 20)
  fused  k_guided_split8 with t0 computed inside it (tuning gf_fuse, window 15): no k_trans_init
  fast   k_guided_fast<TH> (windows the wavefront kernels do not take)
  exact  the k_box_* passes of cv2.boxFilter's order (gf_exact; float64 images); window 15 fuses the first filter's passes
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SMALL, ODD, BANDED = (1, 96, 128), (1, 97, 131), (1, 200, 256)
LARGE, LARGE_ODD = (10, 1080, 1920), (10, 1080, 1919)  # 20.7 MP: a job the split kernel takes


@pytest.fixture(scope="module")
def dev():
    import underwater_image_enhancement_amd as uw

    d = uw.get_device()
    d.profile(True)
    yield d
    d.profile(False)


@pytest.fixture(scope="module")
def frames(dev):
    rng = np.random.default_rng(77)
    return {shape: dev.tensor(rng.integers(0, 256, shape + (3,), dtype=np.uint8)) for shape in (SMALL, ODD, BANDED, LARGE, LARGE_ODD)}


def guided_kernels(dev):
    """{kernel: launches} of the guided filter since the last call, and whether k_trans_init ran."""
    rows = dev.profile_rows()
    return {n: c for n, (_, c) in rows.items() if n.startswith(("k_guided", "k_box"))}, "k_trans_init" in rows


def check_route(got, route, k):
    if route == "exact":
        assert got and all(n.startswith("k_box") for n in got), got
        assert ("k_box_fused_ab<TP>" in got) == (k == 15), got
        return
    want = {"pipe": {"k_guided_pipe": 1}, "split": {"k_guided_split": 1}, "split+": {"k_guided_split": 1, "k_guided_pipe": 1},
            "fused": {"k_guided_split8": 1}, "fast": {"k_guided_fast<TH>": 1}}[route]
    assert got == want, (route, got)


SIX = [
    # (strategy, shape, params, tuning, route)
    (1, SMALL, {}, {}, "pipe"),
    (2, SMALL, {}, {}, "pipe"),
    (3, SMALL, {}, {}, "pipe"),
    (2, ODD, {}, {}, "pipe"),
    (1, ODD, {}, {}, "pipe"),
    (2, LARGE, {}, {}, "split"),
    (1, LARGE, {}, {}, "split+"),
    (3, LARGE, {}, {}, "pipe"),  # window 10: too few strips x bands for the split kernel
    (2, LARGE_ODD, {}, {}, "pipe"),
    (2, SMALL, {"gf_ksize": 7}, {}, "fast"),
    (2, LARGE, {"gf_ksize": 7}, {}, "fast"),
    (2, SMALL, {"gf_exact": 1}, {}, "exact"),
    (1, SMALL, {"gf_exact": 1}, {}, "exact"),
    (2, LARGE, {"gf_exact": 1}, {}, "exact"),
    (2, SMALL, {"inter_dtype": 2}, {}, "pipe"),
    (2, ODD, {"inter_dtype": 2}, {}, "pipe"),
    (2, LARGE, {"inter_dtype": 2}, {}, "split"),
    (1, LARGE, {"inter_dtype": 2}, {}, "split+"),
    (2, SMALL, {"inter_dtype": 1}, {}, "pipe"),
    (2, LARGE, {"inter_dtype": 1}, {}, "pipe"),  # the fixed-point ring has no split form
    (2, LARGE, {"inter_dtype": 1, "gf_eps": 1e-9}, {}, "split"),  # a/b range too wide for fixed point: the float64 ring
    (2, LARGE, {"gf_exact": 1, "inter_dtype": 2}, {}, "exact"),
    (2, LARGE, {}, {"gf_fuse": 1}, "fused"),
    (2, LARGE, {"inter_dtype": 2}, {"gf_fuse": 1}, "fused"),
    (2, LARGE, {"inter_dtype": 1}, {"gf_fuse": 1}, "pipe"),
    (1, LARGE, {}, {"gf_fuse": 1}, "split+"),
    (2, SMALL, {}, {"gf_fuse": 1}, "pipe"),
    (2, SMALL, {}, {"gf_bands": 2}, "split"),
    (1, BANDED, {}, {"gf_bands": 2}, "split+"),
    (3, BANDED, {}, {"gf_bands": 2}, "split+"),
    (2, ODD, {}, {"gf_bands": 2}, "pipe"),
    (2, LARGE, {}, {"gf_split": 0}, "pipe"),
]


@pytest.mark.parametrize("strategy,shape,over,tune,route", SIX)
def test_six_stadigy_routes(dev, frames, strategy, shape, over, tune, route):
    from underwater_image_enhancement_amd import _lib

    p = dev.params(_lib.SURFACE_SIX, strategy, **over)
    dev.profile_rows()
    with dev.tuning(**tune):
        dev.enhance_u8(frames[shape], p)
        got, trans = guided_kernels(dev)
    check_route(got, route, p.gf_ksize)
    assert trans == (route != "fused")


DICT = [
    ("strong_dehazing", SMALL, {}, {}, "pipe"),
    ("medium_dehazing", SMALL, {}, {}, "pipe"),
    ("light_enhancement", SMALL, {}, {}, "pipe"),
    ("strong_dehazing", ODD, {}, {}, "pipe"),
    ("strong_dehazing", LARGE, {}, {}, "split"),
    ("medium_dehazing", LARGE, {}, {}, "split+"),
    ("light_enhancement", LARGE, {}, {}, "pipe"),
    ("strong_dehazing", LARGE, {}, {"gf_fuse": 1}, "fused"),
    ("strong_dehazing", SMALL, {"gf_exact": 1}, {}, "exact"),
    ("medium_dehazing", SMALL, {"gf_exact": 1}, {}, "exact"),
    ("strong_dehazing", SMALL, {"gf_ksize": 7}, {}, "fast"),
    ("strong_dehazing", SMALL, {"inter_dtype": 1}, {}, "pipe"),
    ("strong_dehazing", LARGE, {"inter_dtype": 1}, {}, "split"),  # (the fixed-point ring is the six_stadigy surface's)
    ("strong_dehazing", SMALL, {}, {"gf_bands": 2}, "split"),
]


@pytest.mark.parametrize("name,shape,over,tune,route", DICT)
def test_dict_dehazing_routes(dev, frames, name, shape, over, tune, route):
    from underwater_image_enhancement_amd import _lib

    p = dev.params(_lib.SURFACE_DICT, _lib.DICT_STRATEGIES[name], **over)
    dev.profile_rows()
    with dev.tuning(**tune):
        dev.enhance_u8(frames[shape], p)
        got, trans = guided_kernels(dev)
    check_route(got, route, p.gf_ksize)
    assert trans == (route != "fused")


@pytest.mark.parametrize("shape,k,mode,route", [
    (SMALL, 15, 0, "pipe"), (SMALL, 15, 1, "exact"), (SMALL, 15, 2, "pipe"),
    (LARGE, 15, 0, "split"), (LARGE, 15, 1, "exact"), (LARGE, 15, 2, "pipe"),
    (LARGE, 20, 0, "split+"), (LARGE, 10, 0, "pipe"), (LARGE_ODD, 15, 0, "pipe"),
    (SMALL, 7, 0, "fast"), (SMALL, 7, 1, "exact"), (SMALL, 7, 2, "fast"), (SMALL, 10, 1, "exact"),
])
def test_guided_filter_modes(dev, shape, k, mode, route):
    import torch

    g = torch.Generator(device=dev.torch_device).manual_seed(5)
    gray = torch.randint(0, 256, shape, generator=g, device=dev.torch_device, dtype=torch.uint8)
    t0 = (0.1 + 0.9 * torch.rand(shape, generator=g, device=dev.torch_device)).float()
    dev.profile_rows()
    dev.guided_filter(gray, t0, k, 0.5, exact=mode)
    got, trans = guided_kernels(dev)
    check_route(got, route, k)
    assert not trans


def test_float_image_routes(dev, frames):
    import torch

    from underwater_image_enhancement_amd import _lib

    img = frames[SMALL].float() / 255.0
    for dtype, surface, strategy, over, route in ((torch.float32, _lib.SURFACE_SIX, 2, {}, "pipe"),
                                                  (torch.float32, _lib.SURFACE_SIX, 2, {"gf_exact": 1}, "exact"),
                                                  (torch.float32, _lib.SURFACE_SIX, 2, {"gf_ksize": 7}, "fast"),
                                                  (torch.float32, _lib.SURFACE_DICT, 1, {}, "pipe"),
                                                  (torch.float64, _lib.SURFACE_DICT, 0, {}, "exact"),
                                                  (torch.float64, _lib.SURFACE_DICT, 1, {}, "exact")):
        p = dev.params(surface, strategy, **over)
        dev.profile_rows()
        dev.enhance_float(img.to(dtype).contiguous(), p)
        got, _ = guided_kernels(dev)
        check_route(got, route, p.gf_ksize)


def test_enhance_all_routes(dev, frames):
    """One workspace for six sets: the gf_exact set runs the k_box passes, its neighbours the wavefront kernel."""
    import torch

    from underwater_image_enhancement_amd import _lib

    B, H, W = SMALL
    p6 = (_lib.UwieParams * 6)()
    for k in range(6):
        p6[k] = dev.params(_lib.SURFACE_SIX, k + 1)
    p6[1].gf_exact = 1
    ws = dev.workspace(dev.lib.uwie_workspace_bytes_all(B, H, W, ctypes.cast(p6, ctypes.c_void_p)))
    out = dev.empty((6, B, H, W, 3), torch.uint8)
    dev.profile_rows()
    _lib.check(dev.lib.uwie_enhance_all_u8(dev._ctx, ctypes.c_void_p(frames[SMALL].data_ptr()), ctypes.c_void_p(out.data_ptr()), None,
                                           B, H, W, ctypes.cast(p6, ctypes.c_void_p), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                                           dev.stream()))
    got, trans = guided_kernels(dev)
    assert got.pop("k_guided_pipe") == 2, got  # strategies 1 and 3
    check_route(got, "exact", 15)
    assert trans
