"""The argument checks of uwie_gray_world_u8, which all run before the context is touched and need no device, its workspace
size function and its plan (include/uwie.h)."""
import ctypes

import pytest

import underwater_image_enhancement_amd as uw

E_INVALID, E_WORKSPACE = -1, -2
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    uw.build()
    return uw.load()


def vp(b):
    return ctypes.cast(b, ctypes.c_void_p) if b is not None else None


def call(lib, ctx, d_in, B, H, W, red, blue, max_gain, d_out, d_stats, ws, ws_bytes):
    return lib.uwie_gray_world_u8(vp(ctx), vp(d_in), B, H, W, red, blue, max_gain, vp(d_out), vp(d_stats), vp(ws), ws_bytes, None)


def test_header_constants():
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uwie.h")).read()
    assert int(re.search(r"#define UWIE_E_INVALID \((-?\d+)\)", text).group(1)) == E_INVALID
    assert int(re.search(r"#define UWIE_E_WORKSPACE \((-?\d+)\)", text).group(1)) == E_WORKSPACE
    assert int(re.search(r"#define UWIE_GW_STATS (\d+)", text).group(1)) == uw._lib.GW_STATS == len(uw.GRAY_WORLD_STAT_NAMES)


def test_argument_errors_without_a_gpu(lib):
    # every check precedes the first use of the context and of the device, so host buffers stand in for the pointers
    ctx, d_in, d_out, d_stats, ws = (ctypes.create_string_buffer(32768) for _ in range(5))
    need = lib.uwie_workspace_bytes_gray_world(1, 8, 8)
    assert 0 < need <= 32768
    ok = (1, 8, 8, 1.0, 0.0, 0.0)
    assert call(lib, None, d_in, *ok, d_out, d_stats, ws, need) == E_INVALID
    assert call(lib, ctx, None, *ok, d_out, d_stats, ws, need) == E_INVALID
    assert call(lib, ctx, d_in, *ok, None, None, ws, need) == E_INVALID
    assert b"both NULL" in lib.uwie_last_error()
    for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1, 1 << 15, 1 << 15), (65536, 1, 1)):
        assert call(lib, ctx, d_in, B, H, W, 1.0, 0.0, 0.0, d_out, d_stats, ws, 1 << 40) == E_INVALID, (B, H, W)
    for bad in (-0.25, 1.5, NAN, INF, -INF):
        assert call(lib, ctx, d_in, 1, 8, 8, bad, 0.0, 0.0, d_out, d_stats, ws, need) == E_INVALID, bad
        assert b"red" in lib.uwie_last_error()
        assert call(lib, ctx, d_in, 1, 8, 8, 1.0, bad, 0.0, d_out, d_stats, ws, need) == E_INVALID, bad
        assert b"blue" in lib.uwie_last_error()
    for bad in (0.5, 0.999, 1e-300, -1.0, -2.0, INF, -INF, NAN):
        assert call(lib, ctx, d_in, 1, 8, 8, 1.0, 0.0, bad, d_out, d_stats, ws, need) == E_INVALID, bad
        assert b"max_gain" in lib.uwie_last_error()
    for which in range(3):  # a misaligned base: d_in, d_out (4 bytes), d_stats (8 bytes)
        ptrs = [vp(d_in), vp(d_out), vp(d_stats)]
        ptrs[which] = ctypes.c_void_p(ctypes.addressof((d_in, d_out, d_stats)[which]) + (4 if which == 2 else 2))
        rc = lib.uwie_gray_world_u8(vp(ctx), ptrs[0], 1, 8, 8, 1.0, 0.0, 0.0, ptrs[1], ptrs[2], vp(ws), need, None)
        assert rc == E_INVALID, which
        assert b"aligned" in lib.uwie_last_error()
    # d_out == d_in is allowed; a d_out that overlaps d_in partially is not (8 x 8 x 3 = 192 bytes)
    base = ctypes.addressof(d_in)
    for shift in (4, 188, -4, -188):
        rc = lib.uwie_gray_world_u8(vp(ctx), ctypes.c_void_p(base + 1024), 1, 8, 8, 1.0, 0.0, 0.0, ctypes.c_void_p(base + 1024 + shift),
                                    vp(d_stats), vp(ws), need, None)
        assert rc == E_INVALID, shift
        assert b"overlaps" in lib.uwie_last_error()
    assert call(lib, ctx, d_in, *ok, d_out, d_stats, ws, need - 1) == E_WORKSPACE
    assert call(lib, ctx, d_in, *ok, d_out, d_stats, None, need) == E_WORKSPACE
    assert call(lib, ctx, d_in, *ok, None, d_stats, None, 0) == E_WORKSPACE
    # (in place, and adjacent buffers, pass every check: they get as far as the workspace)
    assert call(lib, ctx, d_in, *ok, d_in, d_stats, ws, 0) == E_WORKSPACE
    rc = lib.uwie_gray_world_u8(vp(ctx), ctypes.c_void_p(base), 1, 8, 8, 1.0, 0.0, 1.0, ctypes.c_void_p(base + 192), None, vp(ws), 0, None)
    assert rc == E_WORKSPACE


def test_workspace_size(lib):
    size = lib.uwie_workspace_bytes_gray_world
    for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1, 1 << 15, 1 << 15), (65536, 1, 1), (-3, 8, 8)):
        assert size(B, H, W) == 0, (B, H, W)
    for H, W in ((1, 1), (270, 480), (1080, 1920)):
        last = 1  # monotone in the batch (the two arrays are rounded up to 256 bytes, so small batches can share a size)
        for B in (1, 2, 3, 8, 64, 65535):
            n = size(B, H, W)
            assert n >= last and n % 256 == 0, (B, H, W)
            last = n
        assert size(64, H, W) > size(1, H, W) and size(65535, H, W) > size(64, H, W)
    block_px, _ = uw._lib.gray_world_plan(1080, 1920)
    blocks = -(-1080 * 1920 // block_px)
    assert size(1, 1080, 1920) == -(-blocks * 32 // 256) * 256 + 256  # a 32-byte row per workgroup of the sum pass, 96 bytes of stats


def test_plan(lib):
    bp, tp = ctypes.c_int(), ctypes.c_int()
    assert lib.uwie_gray_world_plan(8, 8, None, ctypes.byref(tp)) == E_INVALID
    assert lib.uwie_gray_world_plan(0, 8, ctypes.byref(bp), ctypes.byref(tp)) == E_INVALID
    block_px, thread_px = uw._lib.gray_world_plan(8, 8)
    assert (block_px, thread_px) == uw._lib.gray_world_plan(2160, 3840)  # one pair for every frame
    # the sum pass keeps a workgroup's sums, the largest of them sum r * g <= 255 * 255 * block_px, in 32-bit integers
    assert 1 <= block_px <= 66051 and 65025 * block_px < 2 ** 32
    assert thread_px >= 1 and block_px % thread_px == 0
