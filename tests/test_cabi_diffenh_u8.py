"""uwie_diff_enhance_u8's argument checks, which run before any launch and need no device, and its workspace size."""
import ctypes

import pytest

import underwater_image_enhancement_amd as uw

E_INVALID, E_WORKSPACE = -1, -2


@pytest.fixture(scope="module")
def lib():
    uw.build()
    return uw.load()


def call(lib, ctx, d_in, out_u8, out_f32, B, H, W, params, flags, ws, ws_bytes):
    p = lambda b: ctypes.cast(b, ctypes.c_void_p) if b is not None else None  # noqa: E731
    return lib.uwie_diff_enhance_u8(p(ctx), p(d_in), p(out_u8), p(out_f32), B, H, W, p(params), flags, None, p(ws), ws_bytes, None)


def test_argument_errors_are_rejected_without_a_gpu(lib):
    # every check precedes the first use of the context and of the device, so host buffers stand in for the pointers
    buf = [ctypes.create_string_buffer(4096) for _ in range(6)]
    ctx, d_in, o8, o32, par, ws = buf
    need = lib.uwie_workspace_bytes_diff_u8(1, 8, 8)
    assert 0 < need <= 4096
    assert call(lib, None, d_in, o8, o32, 1, 8, 8, par, 3, ws, need) == E_INVALID
    assert call(lib, ctx, None, o8, o32, 1, 8, 8, par, 3, ws, need) == E_INVALID
    assert call(lib, ctx, d_in, o8, o32, 1, 8, 8, None, 3, ws, need) == E_INVALID
    assert call(lib, ctx, d_in, None, None, 1, 8, 8, par, 3, ws, need) == E_INVALID
    assert b"d_out" in lib.uwie_last_error()
    odd = ctypes.c_void_p(ctypes.addressof(d_in) + 1)  # the count pass reads dwords: d_in is 4-byte aligned
    assert lib.uwie_diff_enhance_u8(ctypes.cast(ctx, ctypes.c_void_p), odd, ctypes.cast(o8, ctypes.c_void_p), None, 1, 8, 8,
                                    ctypes.cast(par, ctypes.c_void_p), 3, None, ctypes.cast(ws, ctypes.c_void_p), need, None) == E_INVALID
    assert b"aligned" in lib.uwie_last_error()
    for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1, 1 << 15, 1 << 15)):
        assert call(lib, ctx, d_in, o8, o32, B, H, W, par, 3, ws, need) == E_INVALID, (B, H, W)
    for flags in (4, -1, 8 | 3):
        assert call(lib, ctx, d_in, o8, o32, 1, 8, 8, par, flags, ws, need) == E_INVALID, flags
    assert call(lib, ctx, d_in, o8, o32, 1, 8, 8, par, 3, ws, need - 1) == E_WORKSPACE
    assert call(lib, ctx, d_in, o8, o32, 1, 8, 8, par, 3, None, need) == E_WORKSPACE
    assert call(lib, ctx, d_in, o8, None, 1, 8, 8, par, 3, None, 0) == E_WORKSPACE


def test_workspace_does_not_grow_with_the_frame(lib):
    one = lib.uwie_workspace_bytes_diff_u8(1, 1, 1)
    assert 0 < one <= 8192
    for H, W in ((8, 8), (1080, 1920), (2160, 3840), (1 << 14, 1 << 14)):
        assert lib.uwie_workspace_bytes_diff_u8(1, H, W) == one
    for B in (2, 8, 32):
        assert lib.uwie_workspace_bytes_diff_u8(B, 2160, 3840) <= B * one
    assert lib.uwie_workspace_bytes_diff_u8(0, 8, 8) == 0 and lib.uwie_workspace_bytes_diff_u8(1, 1 << 15, 1 << 15) == 0
