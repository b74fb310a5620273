"""The argument checks of uwie_fusion_u8, which all run before the context is touched and need no device, its workspace size
function, its plan and its host-side table (include/uwie.h)."""
import ctypes

import numpy as np
import pytest

import fusion_cases as K
import fusion_ref as ref
import underwater_image_enhancement_amd as uw

E_INVALID, E_WORKSPACE = -1, -2
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    uw.build()
    return uw.load()


def vp(b):
    return ctypes.cast(b, ctypes.c_void_p) if b is not None else None


def call(lib, ctx, d_in, B, H, W, gamma, levels, gray_shift, d_out, d_in1, d_in2, d_weight, ws, ws_bytes):
    return lib.uwie_fusion_u8(vp(ctx), vp(d_in), B, H, W, gamma, levels, gray_shift, vp(d_out), vp(d_in1), vp(d_in2), vp(d_weight), vp(ws),
                              ws_bytes, None)


def test_argument_errors_without_a_gpu(lib):
    # every check precedes the first use of the context and of the device, so host buffers stand in for the pointers
    ctx, d_in, d_out, d_in1, d_in2, d_w, ws = (ctypes.create_string_buffer(32768) for _ in range(7))
    need = lib.uwie_workspace_bytes_fusion(1, 8, 8, 3)
    assert 0 < need <= 32768
    ok = (1, 8, 8, 2.2, 3, 15)
    outs = (d_out, d_in1, d_in2, d_w)
    assert call(lib, None, d_in, *ok, *outs, ws, need) == E_INVALID
    assert call(lib, ctx, None, *ok, *outs, ws, need) == E_INVALID
    assert call(lib, ctx, d_in, *ok, None, d_in1, d_in2, d_w, ws, need) == E_INVALID
    assert b"d_out" in lib.uwie_last_error()
    for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1, 1 << 15, 1 << 15), (65536, 1, 1)):
        assert call(lib, ctx, d_in, B, H, W, 2.2, 3, 15, *outs, ws, 1 << 40) == E_INVALID, (B, H, W)
    for bad in (0.0, -1.0, 8.5, NAN, INF, -INF):
        assert call(lib, ctx, d_in, 1, 8, 8, bad, 3, 15, *outs, ws, need) == E_INVALID, bad
        assert b"gamma" in lib.uwie_last_error()
    for bad in (0, -1, 9, 100):
        assert call(lib, ctx, d_in, 1, 8, 8, 2.2, bad, 15, *outs, ws, 1 << 40) == E_INVALID, bad
        assert b"levels" in lib.uwie_last_error()
    for bad in (0, 13, 16, 8):
        assert call(lib, ctx, d_in, 1, 8, 8, 2.2, 3, bad, *outs, ws, need) == E_INVALID, bad
        assert b"gray_shift" in lib.uwie_last_error()
    odd = ctypes.c_void_p(ctypes.addressof(d_w) + 4)
    assert lib.uwie_fusion_u8(vp(ctx), vp(d_in), *ok, vp(d_out), None, None, odd, vp(ws), need, None) == E_INVALID
    assert b"aligned" in lib.uwie_last_error()
    # d_out == d_in is allowed; every other overlap among the four byte planes is not (8 x 8 x 3 = 192 bytes)
    base = ctypes.addressof(d_in) + 1024
    at = ctypes.c_void_p
    for shift in (4, 191, -4, -191):
        assert lib.uwie_fusion_u8(vp(ctx), at(base), *ok, at(base + shift), None, None, None, vp(ws), need, None) == E_INVALID, shift
        assert b"overlap" in lib.uwie_last_error()
    for k in range(2):  # d_in1 / d_in2 on d_in, on d_out, on each other
        parts = [None, None]
        parts[k] = at(base)
        assert lib.uwie_fusion_u8(vp(ctx), at(base), *ok, vp(d_out), *parts, None, vp(ws), need, None) == E_INVALID
        parts[k] = vp(d_out)
        assert lib.uwie_fusion_u8(vp(ctx), at(base), *ok, vp(d_out), *parts, None, vp(ws), need, None) == E_INVALID
    assert lib.uwie_fusion_u8(vp(ctx), at(base), *ok, vp(d_out), vp(d_in1), vp(d_in1), None, vp(ws), need, None) == E_INVALID
    assert b"overlap" in lib.uwie_last_error()
    # a short or missing workspace; in place and adjacent planes pass every check and get as far as the workspace
    assert call(lib, ctx, d_in, *ok, *outs, ws, need - 1) == E_WORKSPACE
    assert call(lib, ctx, d_in, *ok, *outs, None, need) == E_WORKSPACE
    assert call(lib, ctx, d_in, *ok, d_out, None, None, None, None, 0) == E_WORKSPACE
    assert call(lib, ctx, d_in, *ok, d_in, None, None, None, ws, 0) == E_WORKSPACE
    assert lib.uwie_fusion_u8(vp(ctx), at(base), *ok, at(base + 192), at(base + 384), at(base - 192), None, vp(ws), 0, None) == E_WORKSPACE
    for gamma in (1e-300, 8.0):
        assert call(lib, ctx, d_in, 1, 8, 8, gamma, 8, 14, *outs, ws, 0) == E_WORKSPACE, gamma


def test_workspace_size(lib):
    size = lib.uwie_workspace_bytes_fusion
    for B, H, W, L in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, -1, 1), (1, 1 << 15, 1 << 15, 1), (65536, 1, 1, 1), (-3, 8, 8, 1), (1, 8, 8, 0),
                       (1, 8, 8, 9), (1, 8, 8, -1)):
        assert size(B, H, W, L) == 0, (B, H, W, L)

    def monotone(values, f):
        got = [f(v) for v in values]
        assert all(n > 0 and n % 256 == 0 for n in got) and got == sorted(got) and got[-1] > got[0], got

    monotone((1, 2, 3, 8, 64, 4096), lambda B: size(B, 33, 47, 4))
    monotone((1, 2, 17, 270, 1080, 2160), lambda H: size(2, H, 480, 6))
    monotone((1, 2, 17, 270, 1080, 3840), lambda W: size(2, 270, W, 6))
    monotone(range(1, 9), lambda L: size(1, 270, 480, L))
    monotone(range(1, 9), lambda L: size(3, 1, 1, L))  # (a coarser level of a 1 x 1 frame is one point more)
    assert size(65535, 1, 1, 8) > size(4096, 1, 1, 8)
    # the layout the header states: per pixel 3 + 8 + 6 bytes, 56 per point of a coarser level, 32 per tile, 64 per frame
    tw, th = uw._lib.fusion_plan(1080, 1920)
    up = lambda n: -(-n // 256) * 256  # noqa: E731
    H, W, want = 1080, 1920, 0
    want += up(-(-W // tw) * -(-H // th) * 32) + up(64) + up(3 * H * W) + up(6 * H * W) + up(8 * H * W)
    for _ in range(1, 6):
        H, W = (H + 1) // 2, (W + 1) // 2
        want += up(8 * H * W) + 2 * up(24 * H * W)
    assert size(1, 1080, 1920, 6) == want


def test_plan(lib):
    tw, th = ctypes.c_int(), ctypes.c_int()
    assert lib.uwie_fusion_plan(8, 8, 1, None, ctypes.byref(th)) == E_INVALID
    assert lib.uwie_fusion_plan(8, 8, 1, ctypes.byref(tw), None) == E_INVALID
    assert lib.uwie_fusion_plan(0, 8, 1, ctypes.byref(tw), ctypes.byref(th)) == E_INVALID
    assert lib.uwie_fusion_plan(8, 8, 0, ctypes.byref(tw), ctypes.byref(th)) == E_INVALID
    assert lib.uwie_fusion_plan(8, 8, 9, ctypes.byref(tw), ctypes.byref(th)) == E_INVALID
    tile = uw._lib.fusion_plan(8, 8, 1)
    assert tile == uw._lib.fusion_plan(2160, 3840, 8) == K.plan()  # one tile for every frame
    # a workgroup's six channel sums are 32-bit: 255 * tile_w * tile_h must fit
    assert tile[0] >= 1 and tile[1] >= 1 and 255 * tile[0] * tile[1] < 2 ** 32


@pytest.mark.parametrize("gamma", K.TABLE_GAMMAS + (1.0,))
def test_table_equals_numpy(lib, gamma):
    got = uw._lib.fusion_table(gamma)
    assert got.dtype == np.uint8 and got.shape == (256,)
    assert np.array_equal(got, ref.table(gamma))
    if gamma == 1.0:
        assert np.array_equal(got, np.arange(256, dtype=np.uint8))


def test_table_argument_errors(lib):
    buf = (ctypes.c_uint8 * 256)()
    assert lib.uwie_fusion_table(2.2, None) == E_INVALID
    for bad in (0.0, -2.2, 8.000001, NAN, INF):
        assert lib.uwie_fusion_table(bad, buf) == E_INVALID, bad
        assert b"gamma" in lib.uwie_last_error()
