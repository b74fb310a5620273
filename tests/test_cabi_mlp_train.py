"""The argument checks of the training entry points (uwie_mlp_trainer_*, uwie_mlp_train_forward, uwie_mlp_backward,
uwie_mlp_adam_step), which run before the context is touched and need no device; their workspace sizes;
and that the header, the library's exports and _lib.py's signatures agree."""
import ctypes
import os
import re
import struct

import pytest

import underwater_image_enhancement_amd as uw
from underwater_image_enhancement_amd import _lib

E_INVALID, E_WORKSPACE = -1, -2
NAMES = ("uwie_mlp_trainer_create", "uwie_mlp_trainer_destroy", "uwie_mlp_train_workspace_bytes", "uwie_mlp_train_forward",
         "uwie_mlp_backward", "uwie_mlp_adam_step", "uwie_mlp_trainer_get", "uwie_mlp_trainer_set", "uwie_mlp_trainer_step_count",
         "uwie_mlp_trainer_set_step_count", "uwie_mlp_trainer_eval")


@pytest.fixture(scope="module")
def lib():
    uw.build()
    return uw.load()


def vp(b):
    return ctypes.cast(b, ctypes.c_void_p) if b is not None else None


def stand_in(device=0, dims=(79, 64, 1), fwd_batch=0):
    """a stand-in trainer: {int device; (padding); int F, H, nb; three pointers; four arrays; partial; step; fwd_batch; scale}"""
    head = struct.pack("i4xiii4x", device, *dims) + bytes(8 * 3) + bytes(8 * 4) + bytes(8) + struct.pack("qif", 0, fwd_batch, 1.0)
    return ctypes.create_string_buffer(head, 256)


def header():
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "uwie.h")).read()


def test_header_exports_and_signatures_agree(lib):
    text = header()
    ctype = {"int": ctypes.c_int, "double": ctypes.c_double, "size_t": ctypes.c_size_t, "uint64_t": ctypes.c_uint64,
             "long long": ctypes.c_longlong}
    for name in NAMES:
        m = re.search(r"^([\w ]+?)\s*\*?\b" + name + r"\(([^;]*)\);", text, re.M)
        assert m, name
        args = [a.strip() for a in " ".join(m.group(2).split()).split(",")]
        sig = _lib.SIGNATURES[name]
        assert len(sig) == len(args), (name, args)
        for a, t in zip(args, sig):
            if "*" in a:
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, a)
            else:
                assert t is ctype[a.rsplit(" ", 1)[0].replace("const ", "")], (name, a)
        ret = m.group(1).strip()
        want = {"int": ctypes.c_int, "void": None, "size_t": ctypes.c_size_t, "long long": ctypes.c_longlong}[ret]
        assert _lib._RESTYPES.get(name, ctypes.c_int) is want, name
        assert getattr(lib, name).restype is want
    for macro, value in (("UWIE_MASKS_GIVEN", _lib.MASKS_GIVEN), ("UWIE_MASKS_DRAWN", _lib.MASKS_DRAWN),
                         ("UWIE_TRAINER_PARAMS", _lib.TRAINER_PARAMS), ("UWIE_TRAINER_GRADS", _lib.TRAINER_GRADS),
                         ("UWIE_TRAINER_EXP_AVG", _lib.TRAINER_EXP_AVG), ("UWIE_TRAINER_EXP_AVG_SQ", _lib.TRAINER_EXP_AVG_SQ)):
        assert int(re.search(r"#define " + macro + r" (\d+)", text).group(1)) == value


def test_workspace_sizes(lib):
    def want(B, H, nb):
        up = lambda n: (n * 4 + 255) // 256 * 256  # noqa: E731 - float buffers, each on a 256-byte boundary
        bh = B * H
        return (up(bh * (nb + 1)) + up(bh * max(nb, 1)) + up(B * H // 2) + up(B * 4) + 3 * up(bh) + up(B * H // 2))

    for B, H, nb in ((4, 64, 1), (1, 256, 3), (70, 256, 3), (2, 1152, 1), (1, 6, 0), (65536, 2, 0)):
        assert lib.uwie_mlp_train_workspace_bytes(B, H, nb) == want(B, H, nb), (B, H, nb)
    for B, H, nb in ((0, 64, 1), (-1, 64, 1), (65537, 64, 1), (4, 63, 1), (4, 1154, 1), (4, 0, 1), (4, 64, -1), (4, 64, 65)):
        assert lib.uwie_mlp_train_workspace_bytes(B, H, nb) == 0, (B, H, nb)


def test_trainer_create_and_state_argument_errors(lib):
    ctx, par, buf = (ctypes.create_string_buffer(4096) for _ in range(3))
    for dims in ((79, 255, 3), (79, 1154, 3), (1153, 256, 3), (0, 256, 3), (79, 0, 3), (79, 256, -1), (79, 256, 65)):
        h = ctypes.c_void_p(1)
        assert lib.uwie_mlp_trainer_create(vp(ctx), vp(par), *dims, ctypes.byref(h)) == E_INVALID, dims
        assert h.value is None  # no handle is left behind
    h = ctypes.c_void_p(1)
    assert lib.uwie_mlp_trainer_create(None, vp(par), 79, 256, 3, ctypes.byref(h)) == E_INVALID
    assert lib.uwie_mlp_trainer_create(vp(ctx), None, 79, 256, 3, ctypes.byref(h)) == E_INVALID
    assert lib.uwie_mlp_trainer_create(vp(ctx), vp(par), 79, 256, 3, None) == E_INVALID
    lib.uwie_mlp_trainer_destroy(None)
    tr = stand_in()
    for fn in (lib.uwie_mlp_trainer_get, lib.uwie_mlp_trainer_set):
        assert fn(None, 0, vp(buf)) == E_INVALID
        assert fn(vp(tr), 0, None) == E_INVALID
        assert fn(vp(tr), -1, vp(buf)) == E_INVALID and fn(vp(tr), 4, vp(buf)) == E_INVALID
        assert fn(vp(tr), 0, ctypes.c_void_p(ctypes.addressof(buf) + 2)) == E_INVALID
        assert b"which" in lib.uwie_last_error()
    assert lib.uwie_mlp_trainer_step_count(None) == -1 and lib.uwie_mlp_trainer_step_count(vp(tr)) == 0
    assert lib.uwie_mlp_trainer_set_step_count(None, 1) == E_INVALID
    assert lib.uwie_mlp_trainer_set_step_count(vp(tr), -1) == E_INVALID
    assert lib.uwie_mlp_trainer_set_step_count(vp(tr), 1 << 32) == E_INVALID
    assert lib.uwie_mlp_trainer_set_step_count(vp(tr), 7) == 0 and lib.uwie_mlp_trainer_step_count(vp(tr)) == 7


def test_train_forward_argument_errors(lib):
    ctx, feat, out, masks, ws = (ctypes.create_string_buffer(8192) for _ in range(5))
    tr = stand_in()
    need = lib.uwie_mlp_train_workspace_bytes(4, 64, 1)
    assert 0 < need <= 8192

    def fwd(c=ctx, t=tr, f=feat, B=4, p=0.3, mode=_lib.MASKS_GIVEN, m=masks, o=out, w=ws, wb=need, f64=1):
        return lib.uwie_mlp_train_forward(vp(c), vp(t), vp(f), f64, B, p, mode, vp(m), 0, vp(o), vp(w), wb, None)

    assert fwd(c=None) == E_INVALID and fwd(t=None) == E_INVALID and fwd(f=None) == E_INVALID and fwd(o=None) == E_INVALID
    for B in (0, -1, 65537):
        assert fwd(B=B, wb=1 << 40) == E_INVALID, B
    assert b"batch" in lib.uwie_last_error()
    odd = ctypes.c_void_p(ctypes.addressof(feat) + 4)  # float64 rows are 8-byte aligned
    assert lib.uwie_mlp_train_forward(vp(ctx), vp(tr), odd, 1, 4, 0.3, 0, vp(masks), 0, vp(out), vp(ws), need, None) == E_INVALID
    assert b"aligned" in lib.uwie_last_error()
    for p in (-0.1, 1.0, 1.5, float("nan")):
        assert fwd(p=p) == E_INVALID, p
    assert b"[0, 1)" in lib.uwie_last_error()
    for mode in (-1, 2):
        assert fwd(mode=mode) == E_INVALID, mode
    assert b"mask_mode" in lib.uwie_last_error()
    assert fwd(m=None) == E_INVALID and b"d_masks" in lib.uwie_last_error()  # given masks at p > 0
    assert fwd(t=stand_in(device=5)) == E_INVALID and b"another device" in lib.uwie_last_error()
    assert fwd(wb=need - 1) == E_WORKSPACE and fwd(w=None) == E_WORKSPACE


def test_backward_adam_and_eval_argument_errors(lib):
    ctx, feat, grad, out, ws = (ctypes.create_string_buffer(8192) for _ in range(5))
    tr = stand_in(fwd_batch=4)
    need = lib.uwie_mlp_train_workspace_bytes(4, 64, 1)

    def bwd(c=ctx, t=tr, f=feat, B=4, g=grad, w=ws, wb=need):
        return lib.uwie_mlp_backward(vp(c), vp(t), vp(f), 0, B, vp(g), vp(w), wb, None)

    assert bwd(c=None) == E_INVALID and bwd(t=None) == E_INVALID and bwd(f=None) == E_INVALID and bwd(g=None) == E_INVALID
    for B in (0, 65537):
        assert bwd(B=B, wb=1 << 40) == E_INVALID
    assert bwd(g=ctypes.c_void_p(ctypes.addressof(grad) + 2)) == E_INVALID and b"aligned" in lib.uwie_last_error()
    assert bwd(B=3) == E_INVALID and b"precedes" in lib.uwie_last_error()  # the forward ran on 4 rows
    assert bwd(t=stand_in()) == E_INVALID and b"precedes" in lib.uwie_last_error()  # no forward at all
    assert bwd(t=stand_in(device=5, fwd_batch=4)) == E_INVALID and b"another device" in lib.uwie_last_error()
    assert bwd(wb=need - 1) == E_WORKSPACE and bwd(w=None) == E_WORKSPACE

    def adam(c=ctx, t=tr, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8, mn=1.0, norm=None):
        return lib.uwie_mlp_adam_step(vp(c), vp(t), lr, b1, b2, eps, mn, norm, None)

    assert adam(c=None) == E_INVALID and adam(t=None) == E_INVALID
    for kw in ({"lr": -1.0}, {"lr": float("inf")}, {"lr": float("nan")}, {"eps": -1e-8}, {"b1": 1.0}, {"b1": -0.1}, {"b2": 1.0},
               {"b2": float("nan")}, {"mn": 0.0}, {"mn": -1.0}, {"mn": float("nan")}):
        assert adam(**kw) == E_INVALID, kw
    assert adam(norm=ctypes.c_void_p(ctypes.addressof(out) + 4)) == E_INVALID and b"d_norm" in lib.uwie_last_error()
    assert adam(t=stand_in(device=5)) == E_INVALID and b"another device" in lib.uwie_last_error()
    assert lib.uwie_mlp_trainer_step_count(vp(tr)) == 0  # a refused step does not count

    need_eval = lib.uwie_mlp_workspace_bytes(4, 64)

    def ev(c=ctx, t=tr, f=feat, B=4, o=out, w=ws, wb=need_eval):
        return lib.uwie_mlp_trainer_eval(vp(c), vp(t), vp(f), 1, B, vp(o), vp(w), wb, None)

    assert ev(c=None) == E_INVALID and ev(t=None) == E_INVALID and ev(f=None) == E_INVALID and ev(o=None) == E_INVALID
    for B in (0, (1 << 20) + 1):
        assert ev(B=B, wb=1 << 40) == E_INVALID
    assert ev(t=stand_in(device=5)) == E_INVALID and b"another device" in lib.uwie_last_error()
    assert ev(wb=need_eval - 1) == E_WORKSPACE and ev(w=None) == E_WORKSPACE
