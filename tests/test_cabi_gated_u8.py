"""The argument checks of uwie_diff_gated_u8 and uwie_mlp_*, which run before the context is touched and need no device,
and their workspace sizes."""
import ctypes
import struct

import pytest

import underwater_image_enhancement_amd as uw

E_INVALID, E_WORKSPACE = -1, -2


@pytest.fixture(scope="module")
def lib():
    uw.build()
    return uw.load()


def vp(b):
    return ctypes.cast(b, ctypes.c_void_p) if b is not None else None


def gated(lib, ctx, d_in, out_u8, out_f32, B, H, W, params, flags, ws, ws_bytes):
    return lib.uwie_diff_gated_u8(vp(ctx), vp(d_in), vp(out_u8), vp(out_f32), B, H, W, vp(params), flags, None, vp(ws), ws_bytes, None)


def test_error_codes_are_the_headers():
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uwie.h")).read()
    assert int(re.search(r"#define UWIE_E_INVALID \((-?\d+)\)", text).group(1)) == E_INVALID
    assert int(re.search(r"#define UWIE_E_WORKSPACE \((-?\d+)\)", text).group(1)) == E_WORKSPACE


def test_diff_gated_u8_argument_errors_without_a_gpu(lib):
    # every check precedes the first use of the context and of the device, so host buffers stand in for the pointers
    buf = [ctypes.create_string_buffer(32768) for _ in range(6)]
    ctx, d_in, o8, o32, par, ws = buf
    need = lib.uwie_workspace_bytes_diff_gated_u8(1)
    assert 0 < need <= 32768
    assert gated(lib, None, d_in, o8, o32, 1, 8, 8, par, 0, ws, need) == E_INVALID
    assert gated(lib, ctx, None, o8, o32, 1, 8, 8, par, 0, ws, need) == E_INVALID
    assert gated(lib, ctx, d_in, o8, o32, 1, 8, 8, None, 0, ws, need) == E_INVALID
    assert gated(lib, ctx, d_in, None, None, 1, 8, 8, par, 0, ws, need) == E_INVALID
    assert b"d_out" in lib.uwie_last_error()
    odd = ctypes.c_void_p(ctypes.addressof(d_in) + 1)  # the count pass reads dwords: d_in is 4-byte aligned
    assert lib.uwie_diff_gated_u8(vp(ctx), odd, vp(o8), None, 1, 8, 8, vp(par), 0, None, vp(ws), need, None) == E_INVALID
    assert b"aligned" in lib.uwie_last_error()
    for B, H, W in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1, 1 << 15, 1 << 15), (65536, 1, 1)):
        assert gated(lib, ctx, d_in, o8, o32, B, H, W, par, 0, ws, 1 << 40) == E_INVALID, (B, H, W)
    for flags in (1, 3, -1):
        assert gated(lib, ctx, d_in, o8, o32, 1, 8, 8, par, flags, ws, need) == E_INVALID, flags
    assert b"flags" in lib.uwie_last_error()
    assert gated(lib, ctx, d_in, o8, o32, 1, 8, 8, par, 0, ws, need - 1) == E_WORKSPACE
    assert gated(lib, ctx, d_in, o8, o32, 1, 8, 8, par, 0, None, need) == E_WORKSPACE
    assert gated(lib, ctx, d_in, None, o32, 1, 8, 8, par, 0, None, 0) == E_WORKSPACE


def test_diff_gated_u8_workspace_depends_on_the_batch_alone(lib):
    one = lib.uwie_workspace_bytes_diff_gated_u8(1)
    assert one == 2 * 768 * 4 + 768  # the histograms and the float table (3072 B each), the byte table (768 B)
    for B in (2, 8, 32):
        assert one < lib.uwie_workspace_bytes_diff_gated_u8(B) <= B * one
    assert lib.uwie_workspace_bytes_diff_gated_u8(0) == 0 and lib.uwie_workspace_bytes_diff_gated_u8(-3) == 0


def test_mlp_argument_errors_without_a_gpu(lib):
    ctx, par, feat, out, ws = (ctypes.create_string_buffer(4096) for _ in range(5))
    h = ctypes.c_void_p(1)
    for dims in ((79, 255, 3), (79, 1154, 3), (1153, 256, 3), (0, 256, 3), (79, 0, 3), (79, 256, -1), (79, 256, 65)):
        h = ctypes.c_void_p(1)
        assert lib.uwie_mlp_create(vp(ctx), vp(par), *dims, ctypes.byref(h)) == E_INVALID, dims
        assert h.value is None  # no handle is left behind
    assert lib.uwie_mlp_create(None, vp(par), 79, 256, 3, ctypes.byref(h)) == E_INVALID
    assert lib.uwie_mlp_create(vp(ctx), None, 79, 256, 3, ctypes.byref(h)) == E_INVALID
    assert lib.uwie_mlp_create(vp(ctx), vp(par), 79, 256, 3, None) == E_INVALID
    lib.uwie_mlp_destroy(None)
    # a stand-in network on the stand-in context's device: {int device; (padding); int F, H, nb; pointers}
    net = ctypes.create_string_buffer(struct.pack("i4xiii", 0, 79, 256, 3), 256)
    need = lib.uwie_mlp_workspace_bytes(4, 256)
    assert need == 4 * 256 * 4 * 3 + 4 * 128 * 4
    fwd = lambda c, n, f, b, o, w, wb: lib.uwie_mlp_forward(vp(c), vp(n), vp(f), 1, b, vp(o), vp(w), wb, None)  # noqa: E731
    assert fwd(None, net, feat, 4, out, ws, need) == E_INVALID
    assert fwd(ctx, None, feat, 4, out, ws, need) == E_INVALID
    assert fwd(ctx, net, None, 4, out, ws, need) == E_INVALID
    assert fwd(ctx, net, feat, 4, None, ws, need) == E_INVALID
    for B in (0, -1, (1 << 20) + 1):
        assert fwd(ctx, net, feat, B, out, ws, 1 << 40) == E_INVALID, B
    assert b"batch" in lib.uwie_last_error()
    odd = ctypes.c_void_p(ctypes.addressof(feat) + 4)  # float64 rows are 8-byte aligned
    assert lib.uwie_mlp_forward(vp(ctx), vp(net), odd, 1, 4, vp(out), vp(ws), need, None) == E_INVALID
    assert b"aligned" in lib.uwie_last_error()
    elsewhere = ctypes.create_string_buffer(struct.pack("i4xiii", 5, 79, 256, 3), 256)
    assert fwd(ctx, elsewhere, feat, 4, out, ws, need) == E_INVALID
    assert b"another device" in lib.uwie_last_error()
    assert fwd(ctx, net, feat, 4, out, ws, need - 1) == E_WORKSPACE
    assert fwd(ctx, net, feat, 4, out, None, need) == E_WORKSPACE


def test_mlp_workspace_sizes(lib):
    assert lib.uwie_mlp_workspace_bytes(1, 256) == 3 * 1024 + 512
    assert lib.uwie_mlp_workspace_bytes(70, 64) == 3 * 70 * 64 * 4 + 70 * 32 * 4
    for batch, hidden in ((0, 256), (1, 255), (1, 1154), (1, 0), ((1 << 20) + 1, 256)):
        assert lib.uwie_mlp_workspace_bytes(batch, hidden) == 0, (batch, hidden)
