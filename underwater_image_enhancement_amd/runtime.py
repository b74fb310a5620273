"""Device runtime: one libuwie context per GPU, torch tensors as the HBM containers.

PyTorch is plumbing here (device memory, streams); every enhancement operation is a
hand-written HIP kernel reached through the C ABI in include/uwie.h.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import UwieParams, check

_FRAME_DESC = np.dtype([("data", "<u8"), ("H", "<i4"), ("W", "<i4")])  # include/uwie.h uwie_frame_desc
_TRACE_DTYPE = np.dtype([("y0", "<i4"), ("x0", "<i4"), ("rows", "<i4"), ("cols", "<i4"), ("score", "<f8", (4,))])


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class _ClosedOnDel:
    """``close()`` when the object is collected; at interpreter shutdown what ``close()`` needs may be gone already."""

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


class Device(_ClosedOnDel):
    """A libuwie context bound to one MI355X.  Not thread-safe; use one per host thread / stream."""

    def __init__(self, device: int = 0):
        if not torch.cuda.is_available():
            raise _lib.UwieError("no ROCm device visible: the enhancement path has no CPU fallback")
        self.lib = _lib.load()
        self.index = int(device)
        self.torch_device = torch.device("cuda", self.index)
        torch.cuda.set_device(self.index)
        handle = ctypes.c_void_p()
        check(self.lib.uwie_create(self.index, ctypes.byref(handle)))
        self._ctx = handle
        self._workspace = None

    def close(self):
        if getattr(self, "_ctx", None):
            torch.cuda.synchronize(self.index)
            self.lib.uwie_destroy(self._ctx)
            self._ctx = None

    # ------------------------------------------------------------------ plumbing
    def stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.index).cuda_stream)

    def workspace(self, nbytes: int):
        if self._workspace is None or self._workspace.numel() < nbytes:
            self._workspace = None
            self._workspace = torch.empty(int(nbytes), dtype=torch.uint8, device=self.torch_device)
        return self._workspace

    def params(self, surface: int, strategy: int, **overrides) -> UwieParams:
        p = UwieParams()
        check(self.lib.uwie_params_init(ctypes.byref(p), surface, strategy))
        for key, value in overrides.items():
            if not hasattr(p, key):
                raise KeyError(key)
            setattr(p, key, value)
        return p

    def _sized_workspace(self, n: int, message: str, fresh: bool = False):
        """The workspace for what a uwie_*workspace_bytes function answered: 0 means arguments out of range (``message``).
        The cached workspace, or with ``fresh`` a tensor of this call's own (one that has to outlive the next call)."""
        if n == 0:
            raise _lib.UwieError(message)
        return torch.empty(int(n), dtype=torch.uint8, device=self.torch_device) if fresh else self.workspace(n)

    def workspace_for(self, B, H, W, p: UwieParams | None = None):
        n = self.lib.uwie_workspace_bytes_ctx(self._ctx, B, H, W, ctypes.byref(p) if p is not None else None)
        return self._sized_workspace(n, "batch/H/W out of range")

    def tensor(self, array, dtype=None):
        t = torch.as_tensor(np.ascontiguousarray(array))
        if dtype is not None:
            t = t.to(dtype)
        return t.to(self.torch_device)

    def empty(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, device=self.torch_device)

    @staticmethod
    def _bhw(img):
        assert img.dim() == 4 and img.shape[-1] == 3 and img.is_contiguous(), "expected contiguous [B,H,W,3]"
        return int(img.shape[0]), int(img.shape[1]), int(img.shape[2])

    # ------------------------------------------------------------------ route selectors (uwie_set_tuning)
    def tune(self, **selectors):
        """Set route selectors of this context (include/uwie.h: gf_split, gf_bands, select_generic, restore_store,
        lin_predict3, lin_cap, lin_no_predict, lin_predict_shift, q_hist, streams, canny_prepass, entry_fuse ...).  The selection / storage / quadtree
        selectors give the same bytes on every route, the gf_* ones the same transmission to 1e-11 (uwie.h); tests force the
        fallback routes with it."""
        for name, value in selectors.items():
            check(self.lib.uwie_set_tuning(self._ctx, name.encode(), int(value)))

    def tuning(self, **selectors):
        """Context manager: ``with dev.tuning(lin_cap=16): ...`` sets the selectors and puts the old values back."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            old = {}
            for name in selectors:
                v = ctypes.c_int()
                check(self.lib.uwie_get_tuning(self._ctx, name.encode(), ctypes.byref(v)))
                old[name] = v.value
            self.tune(**selectors)
            try:
                yield self
            finally:
                self.tune(**old)

        return scope()

    # ------------------------------------------------------------------ device-side self checks (uwie_device_status)
    def check_status(self, allow: int = 0) -> int:
        """Wait for the current stream and raise ``UwieError`` if a kernel found one of its invariants violated since the last
        check (include/uwie.h: UWIE_E_DEVICE) -- the results of those calls are not valid.  ``enhance`` & co. call this when
        they copy results back to the host (they synchronise there anyway); callers that keep tensors on the device call it
        when they synchronise.  Bits in ``allow`` (UWIE_STATUS_*) are returned instead of raised, for a caller that reports
        them itself; any other bit still raises.  The word is cleared either way."""
        bits = ctypes.c_uint32(0)
        rc = self.lib.uwie_device_status(self._ctx, self.stream(), ctypes.byref(bits))
        if rc != 0 and (bits.value == 0 or bits.value & ~allow):
            check(rc)
        return bits.value

    # ------------------------------------------------------------------ per-kernel timing (HIP events on the launch stream)
    def profile(self, on: bool, only: str | None = None):
        """Per-kernel HIP-event timing on/off; ``only`` restricts it to one kernel name (an event pair per launch costs
        stream time, so a whole-job measurement records the one kernel it reports)."""
        check(self.lib.uwie_profile_filter(self._ctx, only.encode() if only else None))
        check(self.lib.uwie_profile_enable(self._ctx, int(bool(on))))

    def profile_rows(self):
        """Synchronise and return {kernel name: (total ms, launches)} recorded since the last call."""
        n = self.lib.uwie_profile_collect(self._ctx)
        if n < 0:
            check(n)
        rows = {}
        name, ms, calls = ctypes.c_char_p(), ctypes.c_double(), ctypes.c_int()
        for i in range(n):
            check(self.lib.uwie_profile_row(self._ctx, i, ctypes.byref(name), ctypes.byref(ms), ctypes.byref(calls)))
            rows[name.value.decode()] = (ms.value, calls.value)
        return rows

    # ------------------------------------------------------------------ whole pipeline
    def enhance_u8(self, frames, p: UwieParams, want_float: bool = False):
        """frames: uint8 cuda tensor [B,H,W,3] -> (uint8 [B,H,W,3], float32 [B,H,W,3] or None)."""
        B, H, W = self._bhw(frames)
        assert frames.dtype == torch.uint8
        ws = self.workspace_for(B, H, W, p)
        out = self.empty((B, H, W, 3), torch.uint8)
        outf = self.empty((B, H, W, 3), torch.float32) if want_float else None
        check(self.lib.uwie_enhance_u8(self._ctx, _ptr(frames), _ptr(out), _ptr(outf), B, H, W, ctypes.byref(p),
                                       _ptr(ws), ws.numel(), self.stream()))
        return out, outf

    def enhance_u8_f64(self, frames, p: UwieParams):
        """Dict surface: uint8 cuda tensor [B,H,W,3] -> (uint8 [B,H,W,3], float64 [B,H,W,3]): the reference's float64 image."""
        B, H, W = self._bhw(frames)
        assert frames.dtype == torch.uint8
        ws = self.workspace_for(B, H, W, p)
        out = self.empty((B, H, W, 3), torch.uint8)
        outf = self.empty((B, H, W, 3), torch.float64)
        check(self.lib.uwie_enhance_u8_f64(self._ctx, _ptr(frames), _ptr(out), _ptr(outf), B, H, W, ctypes.byref(p),
                                           _ptr(ws), ws.numel(), self.stream()))
        return out, outf

    def enhance_percentiles(self, B, H, W, p: UwieParams):
        """The percentiles the last enhance_u8 / enhance_u8_f64 call of this Device (same B, H, W, p, and the same tuning:
        call it inside that call's ``tuning`` scope) stretched with: float64 [B,3,2] (L_low, L_high), or [B,3,4] (lo1, hi1,
        lo2, hi2) for six_stadigy strategy 3.  Reads the Device's kept workspace (uwie_enhance_percentiles); the context
        knows whether its last enhance call was uwie_enhance_u8_f64, which never splits the batch."""
        ws = self.workspace_for(B, H, W, p)
        k = 4 if p.surface == _lib.SURFACE_SIX and p.strategy == 3 else 2
        out = self.empty((B, 3, k), torch.float64)
        check(self.lib.uwie_enhance_percentiles(self._ctx, _ptr(ws), ws.numel(), B, H, W, ctypes.byref(p), _ptr(out),
                                                self.stream()))
        return out

    def enhance_u8_with_percentiles(self, frames, p: UwieParams, want_float: bool = False):
        """enhance_u8, and the percentiles it used: (uint8 [B,H,W,3], float32 or None, float64 [B,3,2 or 4])."""
        out, outf = self.enhance_u8(frames, p, want_float)
        return out, outf, self.enhance_percentiles(*self._bhw(frames), p)

    def enhance_u8_f64_with_percentiles(self, frames, p: UwieParams):
        """enhance_u8_f64, and the percentiles it used: (uint8 [B,H,W,3], float64 [B,H,W,3], float64 [B,3,2])."""
        out, outf = self.enhance_u8_f64(frames, p)
        return out, outf, self.enhance_percentiles(*self._bhw(frames), p)

    def enhance_float(self, img, p: UwieParams, want: str = "native"):
        """General (not u8-derived) float images [B,H,W,3], float32 (either surface) or float64 (dict surface): returns
        (uint8 [B,H,W,3], float image): float32 for the six_stadigy surface, float64 for the dict surface."""
        assert img.dim() == 4 and img.shape[-1] == 3 and img.is_contiguous(), "expected contiguous [B,H,W,3]"
        B, H, W = (int(v) for v in img.shape[:3])
        six = p.surface == _lib.SURFACE_SIX
        eb = 4 if img.dtype == torch.float32 else 8
        ws = self.workspace(self.lib.uwie_workspace_bytes_float(B, H, W, ctypes.byref(p), eb))
        out = self.empty((B, H, W, 3), torch.uint8)
        if img.dtype == torch.float32:
            of32 = self.empty((B, H, W, 3), torch.float32) if six else None
            of64 = None if six else self.empty((B, H, W, 3), torch.float64)
            check(self.lib.uwie_enhance_f32(self._ctx, _ptr(img), _ptr(out), _ptr(of32), _ptr(of64), B, H, W, ctypes.byref(p),
                                            _ptr(ws), ws.numel(), self.stream()))
            return out, (of32 if six else of64)
        assert img.dtype == torch.float64
        of64 = self.empty((B, H, W, 3), torch.float64)
        check(self.lib.uwie_enhance_f64(self._ctx, _ptr(img), _ptr(out), _ptr(of64), B, H, W, ctypes.byref(p), _ptr(ws),
                                        ws.numel(), self.stream()))
        return out, of64

    def cast_classify_f32(self, img):
        B, H, W = (int(v) for v in img.shape[:3])
        kind = self.empty((B,), torch.int32)
        mean = self.empty((B, 3), torch.float32)
        check(self.lib.uwie_cast_classify_f32(self._ctx, _ptr(img), B, H, W, _ptr(kind), _ptr(mean), self.stream()))
        return kind, mean

    def color_correct_f32(self, img, kind):
        B, H, W = (int(v) for v in img.shape[:3])
        out = self.empty((B, H, W, 3), torch.float32)
        check(self.lib.uwie_color_correct_f32(self._ctx, _ptr(img), _ptr(kind), _ptr(out), B, H, W, self.stream()))
        return out

    def enhance_all_u8(self, frames, cast_correct: bool = True, dark_patch: int = 1):
        """frames: uint8 cuda tensor [B,H,W,3] -> (uint8 [6,B,H,W,3] = strategies 1..6, int32 [B] cast kinds).
        ``dark_patch``: uwie_params.dark_patch of the dehazing strategies 1-3 (4-6 have no dark channel)."""
        B, H, W = self._bhw(frames)
        assert frames.dtype == torch.uint8
        p6 = (UwieParams * 6)()
        for k in range(6):
            p6[k] = self.params(_lib.SURFACE_SIX, k + 1, cast_correct=int(bool(cast_correct)), dark_patch=int(dark_patch) if k < 3 else 1)
        ws = self.workspace(self.lib.uwie_workspace_bytes_all(B, H, W, ctypes.cast(p6, ctypes.c_void_p)))
        out = self.empty((6, B, H, W, 3), torch.uint8)
        kind = self.empty((B,), torch.int32)
        check(self.lib.uwie_enhance_all_u8(self._ctx, _ptr(frames), _ptr(out), _ptr(kind), B, H, W,
                                           ctypes.cast(p6, ctypes.c_void_p), _ptr(ws), ws.numel(), self.stream()))
        return out, kind

    # ------------------------------------------------------------------ the enhancement modules (uwie_diff_*, DESIGN.md sections 8, 10)
    @staticmethod
    def _module_args(img, params, planar: bool, *same):
        """The common front of the module bindings: img float32 [B,3,H,W] (planar) or [B,H,W,3], params float32 [B,4] (or
        None), ``same``: float32 tensors of img's shape (or None).  Returns ((B, H, W), the tensors made contiguous)."""
        assert img.dtype == torch.float32 and img.dim() == 4 and img.shape[1 if planar else 3] == 3
        B = int(img.shape[0])
        H, W = (int(v) for v in (img.shape[2:] if planar else img.shape[1:3]))
        assert params is None or (params.dtype == torch.float32 and tuple(params.shape) == (B, 4))
        assert all(t is None or (t.dtype == torch.float32 and tuple(t.shape) == tuple(img.shape)) for t in same)
        return (B, H, W), [t if t is None else t.contiguous() for t in (img, params) + same]

    def _module_fwd(self, fn, img, params, planar: bool, flags: int, save: bool):
        """A module forward (fn = uwie_diff_*_f32) or, with ``save``, its _save_f32 form, which also fills saved [B,3,2]."""
        (B, H, W), (img, params) = self._module_args(img, params, planar)
        ws = self.workspace_for(B, H, W)
        out = self.empty(tuple(img.shape), torch.float32)
        saved = self.empty((B, 3, 2), torch.float32) if save else None
        check(fn(self._ctx, _ptr(img), _ptr(out), B, H, W, int(planar), _ptr(params), int(flags),
                 *((_ptr(saved),) if save else ()), _ptr(ws), ws.numel(), self.stream()))
        return (out, saved) if save else out

    def _module_bwd(self, fn, ws_bytes, img, params, saved, grad_out, planar: bool, flags: int, want_img: bool):
        """A module backward (fn = uwie_diff_*_bwd_f32, ws_bytes its workspace function): (grad_img or None, grad_params)."""
        (B, H, W), (img, params, grad_out) = self._module_args(img, params, planar, grad_out)
        ws = self.workspace(ws_bytes(B, H, W))
        grad_img = self.empty(tuple(img.shape), torch.float32) if want_img else None
        grad_params = self.empty((B, 4), torch.float32)
        check(fn(self._ctx, _ptr(img), _ptr(params), int(flags), int(planar), B, H, W, _ptr(saved.contiguous()), _ptr(grad_out),
                 _ptr(grad_img), _ptr(grad_params), _ptr(ws), ws.numel(), self.stream()))
        return grad_img, grad_params

    def diff_enhance_f32(self, img, params, planar: bool, has_omega: bool = True, has_gamma: bool = True):
        """img: float32 cuda tensor [B,3,H,W] (planar) or [B,H,W,3]; params: float32 [B,4] = L_low, L_high, omega, gamma."""
        flags = (1 if has_omega else 0) | (2 if has_gamma else 0)
        return self._module_fwd(self.lib.uwie_diff_enhance_f32, img, params, planar, flags, False)

    def diff_enhance_save_f32(self, img, params, planar: bool, flags: int):
        """diff_enhance_f32 that also returns what the backward needs: (out, saved float32 [B,3,2] = p_lo, p_hi per plane)."""
        return self._module_fwd(self.lib.uwie_diff_enhance_save_f32, img, params, planar, flags, True)

    def diff_enhance_bwd_f32(self, img, params, saved, grad_out, planar: bool, flags: int, want_img: bool = True):
        """Gradient of diff_enhance: (grad_img in img's layout or None when not wanted, grad_params float32 [B,4] =
        0, 0, d omega, d gamma)."""
        return self._module_bwd(self.lib.uwie_diff_enhance_bwd_f32, self.lib.uwie_diff_enhance_bwd_workspace_bytes, img, params,
                                saved, grad_out, planar, flags, want_img)

    def _module_u8(self, fn, ws_bytes, ws_message: str, u8, cols, flags: int, want_u8: bool, want_f32: bool, saved: bool):
        """A module in the byte domain (fn = uwie_diff_*_u8, ws_bytes = its workspace size for (B, H, W))."""
        assert u8.dtype == torch.uint8
        u8 = u8.contiguous()
        B, H, W = self._bhw(u8)
        assert cols.dtype == torch.float32 and tuple(cols.shape) == (B, 4)
        cols = cols.contiguous()
        ws = self._sized_workspace(ws_bytes(B, H, W), ws_message)
        out_u8 = self.empty((B, H, W, 3), torch.uint8) if want_u8 else None
        out_f32 = self.empty((B, H, W, 3), torch.float32) if want_f32 else None
        sv = self.empty((B, 3, 2), torch.float32) if saved else None
        check(fn(self._ctx, _ptr(u8), _ptr(out_u8), _ptr(out_f32), B, H, W, _ptr(cols), int(flags), _ptr(sv), _ptr(ws), ws.numel(),
                 self.stream()))
        return (out_u8, out_f32, sv) if saved else (out_u8, out_f32)

    def diff_enhance_u8(self, u8, cols, flags: int = 3, want_u8: bool = True, want_f32: bool = False, saved: bool = False):
        """The module in the byte domain (uwie_diff_enhance_u8).  u8: uint8 cuda tensor [B,H,W,3], the
        frame whose float image is u8 / 255; cols: float32 [B,4] = L_low, L_high, omega, gamma.  Returns (out_u8 or None =
        (uint8)(v * 255) of the module's output v, out_f32 or None = v, the bits diff_enhance_f32 gives for u8_to_f32(u8)),
        and with ``saved`` a third item, float32 [B,3,2] as diff_enhance_save_f32 returns it."""
        return self._module_u8(self.lib.uwie_diff_enhance_u8, self.lib.uwie_workspace_bytes_diff_u8, "batch/H/W out of range",
                               u8, cols, flags, want_u8, want_f32, saved)

    def diff_gated_f32(self, img, params, planar: bool):
        """deep_learning_parameters.DifferentiableEnhancement's forward (uwie_diff_gated_f32): img float32 cuda [B,3,H,W]
        (planar) or [B,H,W,3]; params float32 [B,4] = L_low, L_high, use_gamma, gamma.  An image without a valid sorted
        position gets NaN and sets UWIE_STATUS_DIFF_RANK (check_status)."""
        return self._module_fwd(self.lib.uwie_diff_gated_f32, img, params, planar, 0, False)

    def diff_gated_save_f32(self, img, params, planar: bool):
        """diff_gated_f32 that also returns what the backward needs: (out, saved float32 [B,3,2] = p_lo, p_hi per plane)."""
        return self._module_fwd(self.lib.uwie_diff_gated_save_f32, img, params, planar, 0, True)

    def diff_gated_bwd_f32(self, img, params, saved, grad_out, planar: bool, want_img: bool = True):
        """Gradient of diff_gated: (grad_img in img's layout or None when not wanted, grad_params float32 [B,4] =
        0, 0, d use_gamma, d gamma)."""
        return self._module_bwd(self.lib.uwie_diff_gated_bwd_f32, self.lib.uwie_diff_gated_bwd_workspace_bytes, img, params,
                                saved, grad_out, planar, 0, want_img)

    def diff_gated_u8(self, u8, cols, want_u8: bool = True, want_f32: bool = False, saved: bool = False):
        """The gated module in the byte domain (uwie_diff_gated_u8).  u8: uint8 cuda tensor [B,H,W,3], the
        frame whose float image is u8 / 255; cols: float32 [B,4] = L_low, L_high, use_gamma, gamma.  Returns (out_u8 or None =
        (uint8)(v * 255) of the module's output v, out_f32 or None = v, the bits diff_gated_f32 gives for u8_to_f32(u8)), and
        with ``saved`` a third item, float32 [B,3,2] as diff_gated_save_f32 returns it.  An image without a valid sorted
        position gets NaN / 0 and sets UWIE_STATUS_DIFF_RANK (check_status)."""
        return self._module_u8(self.lib.uwie_diff_gated_u8, lambda B, H, W: self.lib.uwie_workspace_bytes_diff_gated_u8(B),
                               "batch out of range", u8, cols, 0, want_u8, want_f32, saved)

    # ------------------------------------------------------------------ ReferenceLoss (uwie_ref_loss_*)
    def ref_loss_f32(self, map_: int, img, params, ref, planar: bool, flags: int = 0, want_out: bool = False,
                     status: bool = False):
        """l1, l2 of o (map_: _lib.LOSS_IDENTITY: o = img; LOSS_VGG / LOSS_GATED: the module's output of img, params) against
        ref.  Returns (out or None, saved float32 [B,3,2] or None (identity), buf float32 [4]): buf[0], buf[1] = l1, l2 and,
        with ``status``, buf[2] = the device status word (uwie_device_status_async, cleared on the device) as uint32 bits, so
        that one copy brings back all three."""
        identity = map_ == _lib.LOSS_IDENTITY
        assert identity or params is not None
        (B, H, W), (img, params, ref) = self._module_args(img, None if identity else params, planar, ref)
        ws = self.workspace(self.lib.uwie_ref_loss_workspace_bytes(B, H, W))
        buf = self.empty((4,), torch.float32)
        saved = None if identity else self.empty((B, 3, 2), torch.float32)
        out = self.empty(tuple(img.shape), torch.float32) if want_out and not identity else None
        check(self.lib.uwie_ref_loss_f32(self._ctx, int(map_), _ptr(img), _ptr(params), int(flags), int(planar), B, H, W, _ptr(ref),
                                         _ptr(out), _ptr(saved), _ptr(buf), _ptr(ws), ws.numel(), self.stream()))
        if status:
            check(self.lib.uwie_device_status_async(self._ctx, ctypes.c_void_p(buf.data_ptr() + 8), self.stream()))
        return out, saved, buf

    def ref_loss_bwd_f32(self, map_: int, img, params, saved, ref, grad_loss, planar: bool, flags: int = 0, grad_out=None,
                         want_img: bool = True):
        """Gradient of ref_loss_f32 given grad_loss float32 [2] = dL/dl1, dL/dl2 on the device (and grad_out = dL/d(out) when
        the output was kept and used): (grad_img or None, grad_params float32 [B,4] or None for the identity map)."""
        identity = map_ == _lib.LOSS_IDENTITY
        (B, H, W), (img, params, ref, grad_out) = self._module_args(img, None if identity else params, planar, ref, grad_out)
        grad_loss = grad_loss.contiguous()
        assert grad_loss.dtype == torch.float32 and grad_loss.numel() == 2
        ws = self.workspace(self.lib.uwie_ref_loss_workspace_bytes(B, H, W))
        grad_img = self.empty(tuple(img.shape), torch.float32) if want_img or identity else None
        grad_params = None if identity else self.empty((B, 4), torch.float32)
        check(self.lib.uwie_ref_loss_bwd_f32(self._ctx, int(map_), _ptr(img), _ptr(params), int(flags), int(planar), B, H, W,
                                             _ptr(saved), _ptr(ref), _ptr(grad_out), _ptr(grad_loss), _ptr(grad_img),
                                             _ptr(grad_params), _ptr(ws), ws.numel(), self.stream()))
        return grad_img, grad_params

    # ------------------------------------------------------------------ PerceptualLoss (uwie_perceptual_*)
    def _net_create(self, fn, params, count: int, *args):
        """A handle from fn = uwie_*_create(ctx, the ``count`` flat float32 parameters, *args, &handle).  The caller owns it."""
        flat = params.to(device=self.torch_device, dtype=torch.float32).contiguous()
        assert flat.numel() == count
        torch.cuda.synchronize(self.index)  # the packing runs on the null stream
        handle = ctypes.c_void_p()
        check(fn(self._ctx, _ptr(flat), *args, ctypes.byref(handle)))
        return handle

    def _net_destroy(self, fn, handle):
        torch.cuda.synchronize(self.index)  # work in flight may still read the handle's arrays
        fn(handle)

    def vgg_create(self, params, precision: int):
        """A uwie_vgg handle of ``precision`` (_lib.VGG_F32 / VGG_F16) from torchvision's 14 tensors flattened in features.N
        order (float32, _lib.VGG_PARAMS values).  The caller owns it (vgg_destroy)."""
        return self._net_create(self.lib.uwie_vgg_create, params, _lib.VGG_PARAMS, int(precision))

    def vgg_destroy(self, handle):
        self._net_destroy(self.lib.uwie_vgg_destroy, handle)

    def perceptual_f32(self, vgg, precision: int, pred, target):
        """mse_loss(F(pred), F(target)) on the device.  Returns (buf float32 [1] = the loss, ws = this call's workspace, which
        holds what perceptual_bwd_f32 needs: keep it untouched until then).  The perceptual kernels set no status bit, so
        this call neither reads nor clears the device status word: bits pending from earlier calls stay for their checks."""
        assert pred.dtype == torch.float32 and target.dtype == torch.float32 and pred.dim() == 4 and pred.shape[1] == 3
        assert tuple(pred.shape) == tuple(target.shape)
        B, _, H, W = (int(v) for v in pred.shape)
        ws = self._sized_workspace(self.lib.uwie_perceptual_workspace_bytes(B, H, W, int(precision)),
                                   f"perceptual: batch/H/W out of range ({B}, {H}, {W})", fresh=True)
        buf = self.empty((1,), torch.float32)
        check(self.lib.uwie_perceptual_f32(self._ctx, vgg, _ptr(pred.contiguous()), _ptr(target.contiguous()), B, H, W, _ptr(buf),
                                           _ptr(ws), ws.numel(), self.stream()))
        return buf, ws

    def perceptual_bwd_f32(self, vgg, shape, ws, grad_loss):
        """dloss/dpred * grad_loss (float32 [1] on the device) from the workspace of perceptual_f32: float32 ``shape``."""
        B, _, H, W = (int(v) for v in shape)
        grad_loss = grad_loss.to(device=self.torch_device, dtype=torch.float32).reshape(1).contiguous()
        out = self.empty(tuple(shape), torch.float32)
        check(self.lib.uwie_perceptual_bwd_f32(self._ctx, vgg, B, H, W, _ptr(grad_loss), _ptr(out), _ptr(ws), ws.numel(),
                                               self.stream()))
        return out

    # ------------------------------------------------------------------ ImprovedVGGParameterNet (uwie_param_net_*)
    def param_net_create(self, params, use_features: bool):
        """A uwie_param_net handle from the state dict's float tensors flattened in state-dict order (float32,
        _lib.PARAM_NET_PARAMS[use_features] values; include/uwie.h lists the order).  The caller owns it (param_net_destroy)."""
        return self._net_create(self.lib.uwie_param_net_create, params, _lib.PARAM_NET_PARAMS[bool(use_features)],
                                int(bool(use_features)))

    def param_net_destroy(self, handle):
        self._net_destroy(self.lib.uwie_param_net_destroy, handle)

    def param_net_f32(self, net, img, features=None, want_pooled: bool = False):
        """The eval-mode forward: img float32 cuda [B,3,H,W], features float32 cuda [B,79] or None.  Returns (float32 [B,4] =
        omega, gamma, L_low, L_high, float32 [B,1024] pooled vector or None).  Sets no status bit."""
        assert img.dtype == torch.float32 and img.dim() == 4 and img.shape[1] == 3
        B, _, H, W = (int(v) for v in img.shape)
        if features is not None:
            assert features.dtype == torch.float32 and tuple(features.shape) == (B, 79)
            features = features.contiguous()
        ws = self._sized_workspace(self.lib.uwie_param_net_workspace_bytes(B, H, W),
                                   f"param_net: batch/H/W out of range ({B}, {H}, {W})", fresh=True)
        out = self.empty((B, 4), torch.float32)
        pooled = self.empty((B, 1024), torch.float32) if want_pooled else None
        check(self.lib.uwie_param_net_f32(self._ctx, net, _ptr(img.contiguous()), _ptr(features), B, H, W, _ptr(out), _ptr(pooled),
                                          _ptr(ws), ws.numel(), self.stream()))
        return out, pooled

    # ------------------------------------------------------------------ ParameterPredictor (uwie_mlp_*)
    @staticmethod
    def mlp_param_count(feature_dim: int, hidden_dim: int, num_blocks: int) -> int:
        """The values of a ParameterPredictor's state_dict(): input layer, the blocks' two layers each, the neck, four heads."""
        f, h, half = int(feature_dim), int(hidden_dim), int(hidden_dim) // 2
        return f * h + h + int(num_blocks) * 2 * (h * h + h) + half * h + half + 4 * (half + 1)

    def _mlp_create(self, fn, params, feature_dim: int, hidden_dim: int, num_blocks: int):
        dims = (int(feature_dim), int(hidden_dim), int(num_blocks))
        return self._net_create(fn, params, self.mlp_param_count(*dims), *dims)

    def mlp_create(self, params, feature_dim: int, hidden_dim: int, num_blocks: int):
        """A uwie_mlp handle from the state dict's tensors flattened in state_dict() order (float32; include/uwie.h lists
        the order).  The caller owns it (mlp_destroy)."""
        return self._mlp_create(self.lib.uwie_mlp_create, params, feature_dim, hidden_dim, num_blocks)

    def mlp_destroy(self, handle):
        self._net_destroy(self.lib.uwie_mlp_destroy, handle)

    def _mlp_eval(self, fn, who: str, handle, rows, hidden_dim: int):
        """fn = uwie_mlp_forward or uwie_mlp_trainer_eval on its handle."""
        assert rows.dtype in (torch.float32, torch.float64) and rows.dim() == 2
        rows = rows.contiguous()
        B = int(rows.shape[0])
        ws = self._sized_workspace(self.lib.uwie_mlp_workspace_bytes(B, int(hidden_dim)), f"{who}: batch out of range ({B})",
                                   fresh=True)
        out = self.empty((B, 4), torch.float32)
        check(fn(self._ctx, handle, _ptr(rows), int(rows.dtype == torch.float64), B, _ptr(out), _ptr(ws), ws.numel(), self.stream()))
        return out

    def mlp_forward(self, net, rows, hidden_dim: int):
        """The eval-mode forward: rows float64 or float32 cuda [B, feature_dim] (float64 is rounded to float32 on load).
        Returns float32 [B,4] = L_low, L_high, use_gamma, gamma.  Sets no status bit."""
        return self._mlp_eval(self.lib.uwie_mlp_forward, "mlp_forward", net, rows, hidden_dim)

    # ------------------------------------------------------------------ EndToEndTrainer's step (uwie_mlp_trainer_*)
    def mlp_trainer_create(self, params, feature_dim: int, hidden_dim: int, num_blocks: int):
        """A uwie_mlp_trainer handle from the flat state_dict()-order parameters, as mlp_create.  The caller owns it."""
        return self._mlp_create(self.lib.uwie_mlp_trainer_create, params, feature_dim, hidden_dim, num_blocks)

    def mlp_trainer_destroy(self, handle):
        self._net_destroy(self.lib.uwie_mlp_trainer_destroy, handle)

    def mlp_train_workspace(self, B: int, hidden_dim: int, num_blocks: int):
        return self._sized_workspace(self.lib.uwie_mlp_train_workspace_bytes(int(B), int(hidden_dim), int(num_blocks)),
                                     f"mlp_train: batch out of range ({B})", fresh=True)

    def mlp_train_forward(self, tr, rows, ws, p: float, masks=None, seed: int = 0, want_masks=None):
        """The train-mode forward: rows as mlp_forward; ws from mlp_train_workspace (the backward reads it).  masks: uint8 cuda
        [sites, B, hidden] (given), or None: drawn from (seed, the trainer's step count), written to want_masks (a uint8
        tensor of that shape) when it is not None.  Returns float32 [B,4] = L_low, L_high, use_gamma, gamma."""
        assert rows.dtype in (torch.float32, torch.float64) and rows.dim() == 2 and rows.is_contiguous()
        B = int(rows.shape[0])
        out = self.empty((B, 4), torch.float32)
        if masks is not None:
            assert masks.dtype == torch.uint8 and masks.is_contiguous() and masks.dim() == 3 and masks.shape[1] == B
            mode, mptr = _lib.MASKS_GIVEN, _ptr(masks)
        else:
            assert want_masks is None or (want_masks.dtype == torch.uint8 and want_masks.is_contiguous() and want_masks.shape[1] == B)
            mode, mptr = _lib.MASKS_DRAWN, _ptr(want_masks)
        check(self.lib.uwie_mlp_train_forward(self._ctx, tr, _ptr(rows), int(rows.dtype == torch.float64), B, float(p), mode, mptr,
                                              int(seed) & (2**64 - 1), _ptr(out), _ptr(ws), ws.numel(), self.stream()))
        return out

    def mlp_backward(self, tr, rows, ws, grad_out):
        """The MLP's backward of the last mlp_train_forward (same rows and ws): grad_out float32 cuda [B,4] in the gated order
        (its first two columns are not read).  Overwrites the trainer's gradients."""
        assert grad_out.dtype == torch.float32 and tuple(grad_out.shape) == (rows.shape[0], 4) and grad_out.is_contiguous()
        check(self.lib.uwie_mlp_backward(self._ctx, tr, _ptr(rows), int(rows.dtype == torch.float64), int(rows.shape[0]),
                                         _ptr(grad_out), _ptr(ws), ws.numel(), self.stream()))

    def mlp_adam_step(self, tr, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, max_norm=1.0, norm=None):
        """clip_grad_norm_(max_norm) and one torch.optim.Adam step on the trainer's arrays; norm: a float64 cuda [1] that
        receives total_norm, or None.  No host read."""
        assert norm is None or (norm.dtype == torch.float64 and norm.numel() == 1)
        check(self.lib.uwie_mlp_adam_step(self._ctx, tr, float(lr), float(betas[0]), float(betas[1]), float(eps), float(max_norm),
                                          _ptr(norm), self.stream()))

    def mlp_trainer_get(self, tr, which: int, count: int):
        """One of the trainer's arrays (_lib.TRAINER_*) as a float32 cuda [count] in state_dict() order."""
        buf = self.empty((int(count),), torch.float32)
        check(self.lib.uwie_mlp_trainer_get(tr, int(which), _ptr(buf)))
        return buf

    def mlp_trainer_set(self, tr, which: int, flat):
        flat = flat.to(device=self.torch_device, dtype=torch.float32).contiguous()
        torch.cuda.synchronize(self.index)
        check(self.lib.uwie_mlp_trainer_set(tr, int(which), _ptr(flat)))

    def mlp_trainer_eval(self, tr, rows, hidden_dim: int):
        """mlp_forward on the trainer's current weights."""
        return self._mlp_eval(self.lib.uwie_mlp_trainer_eval, "mlp_trainer_eval", tr, rows, hidden_dim)

    def u8_to_f32(self, frames):
        """uint8 cuda tensor of any shape -> float32 of that shape, u8.astype(float32) / 255.0 (uwie_u8_to_f32)."""
        assert frames.dtype == torch.uint8
        frames = frames.contiguous()
        out = self.empty(tuple(frames.shape), torch.float32)
        check(self.lib.uwie_u8_to_f32(self._ctx, _ptr(frames), _ptr(out), frames.numel(), self.stream()))
        return out

    def extract_features_u8(self, frames):
        """frames: uint8 cuda tensor [B,H,W,3] -> float32 [B,79] (vgg_16_UIE.extract_all_features per frame)."""
        B, H, W = self._bhw(frames)
        assert frames.dtype == torch.uint8
        ws = self.workspace_for(B, H, W)
        out = self.empty((B, 79), torch.float32)
        check(self.lib.uwie_extract_features_u8(self._ctx, _ptr(frames), _ptr(out), B, H, W, _ptr(ws), ws.numel(),
                                                self.stream()))
        return out

    def feature_extractor(self, frames_u8, frames_f32=None, gray_shift: int = 15):
        """feature_extraction.FeatureExtractor.extract_all_features per frame (uwie_feature_extractor_u8): frames_u8 uint8 cuda
        [B,H,W,3] (the quantised image), frames_f32 optional float32 cuda [B,H,W,3] (read by the RGB block only).  Returns
        float64 [B,79], or [B,74] when H or W is odd and > 1 (no DCT block, as the reference)."""
        B, H, W = self._bhw(frames_u8)
        assert frames_u8.dtype == torch.uint8
        if frames_f32 is not None:
            assert frames_f32.dtype == torch.float32 and tuple(frames_f32.shape) == (B, H, W, 3)
            frames_f32 = frames_f32.contiguous()
        nbytes = self.lib.uwie_workspace_bytes_feature_extractor(B, H, W)
        if nbytes == 0:
            raise _lib.UwieError("feature_extractor: batch/H/W out of range")
        ws = self.workspace(nbytes)
        out = self.empty((B, self.lib.uwie_feature_extractor_count(H, W)), torch.float64)
        check(self.lib.uwie_feature_extractor_u8(self._ctx, _ptr(frames_u8), _ptr(frames_f32), B, H, W, int(gray_shift), _ptr(out),
                                                 _ptr(ws), ws.numel(), self.stream()))
        return out

    def frame_table(self, frames):
        """Device descriptor table (uwie_frame_desc) of RGB u8 frames: a contiguous [B,H,W,3] tensor on this device, or a list
        of [H,W,3] frames that are all host NumPy arrays (packed into one pinned buffer, one upload) or all tensors on this
        device (their own pointers, no copy).  Returns (table, (keep, sizes)): ``keep`` is the memory the table points to.
        Uploads go on the current stream, the launch that reads them too: the caching allocators may release them after it."""
        if isinstance(frames, torch.Tensor):
            B, H, W = self._bhw(frames)
            assert frames.dtype == torch.uint8 and frames.device == self.torch_device
            sizes = [(H, W)] * B
            base, step = frames.data_ptr(), H * W * 3
            ptrs = [base + i * step for i in range(B)]
            keep = frames
        else:
            frames = list(frames)
            if not frames:
                raise ValueError("empty frame list")
            on_host = [isinstance(f, np.ndarray) for f in frames]
            if any(on_host) and not all(on_host):
                raise TypeError("a frame list is either all host NumPy arrays or all device tensors")
            for f in frames:
                if f.dtype not in (np.uint8, torch.uint8):
                    raise TypeError(f"expected uint8 frames, got {f.dtype}")
                if f.ndim != 3 or f.shape[2] != 3:
                    raise ValueError(f"expected [H,W,3] frames, got {tuple(f.shape)}")
            sizes = [(int(f.shape[0]), int(f.shape[1])) for f in frames]
            if all(on_host):
                offs = np.cumsum([0] + [h * w * 3 for h, w in sizes])
                pinned = torch.empty(int(offs[-1]), dtype=torch.uint8, pin_memory=True)
                host = pinned.numpy()
                for f, o0, o1 in zip(frames, offs[:-1], offs[1:]):
                    host[o0:o1] = np.ascontiguousarray(f).reshape(-1)
                keep = pinned.to(self.torch_device, non_blocking=True)
                ptrs = [keep.data_ptr() + int(o) for o in offs[:-1]]
            else:
                for f in frames:
                    if f.device != self.torch_device or not f.is_contiguous():
                        raise ValueError("device frames must be contiguous tensors on this device")
                keep = frames
                ptrs = [f.data_ptr() for f in frames]
        for h, w in sizes:
            if not (1 <= h <= _lib.RESIZE_MAX_SRC and 1 <= w <= _lib.RESIZE_MAX_SRC):
                raise ValueError(f"frame size {h}x{w} outside [1, {_lib.RESIZE_MAX_SRC}]")
        table = np.zeros(len(sizes), _FRAME_DESC)
        table["data"], table["H"], table["W"] = ptrs, [h for h, _ in sizes], [w for _, w in sizes]
        dt = torch.from_numpy(table.view(np.uint8)).pin_memory().to(self.torch_device, non_blocking=True)
        return dt, (keep, sizes)

    def resize_rgb(self, frames, out_h: int, out_w: int, flips=None, want_u8: bool = True, want_f32: bool = False, norm=None):
        """cv2.resize(frame, (out_w, out_h)) of every frame in one launch (uwie_resize_rgb_u8).  ``frames``: see frame_table
        (frames may differ in size).  ``flips``: per-frame flags (1 = fliplr, 2 = flipud of the result) or None.
        ``norm``: (mean3, std3) for the normalised planes, or None.  Returns (u8 [B,oh,ow,3] or None, float32 [B,3,oh,ow] =
        v / 255 or None, normalised float32 [B,3,oh,ow] or None)."""
        table, keep = self.frame_table(frames)
        B = len(keep[1])
        f = None
        if flips is not None:
            fl = np.asarray(flips, dtype=np.int64).reshape(-1)
            if fl.size != B or np.any((fl < 0) | (fl > 3)):
                raise ValueError("flips: one value in 0..3 per frame")
            f = torch.from_numpy(fl.astype(np.uint8)).to(self.torch_device)
        u8 = self.empty((B, out_h, out_w, 3), torch.uint8) if want_u8 else None
        f32 = self.empty((B, 3, out_h, out_w), torch.float32) if want_f32 else None
        nrm = m = s = None
        if norm is not None:
            nrm = self.empty((B, 3, out_h, out_w), torch.float32)
            m = (ctypes.c_float * 3)(*[float(v) for v in norm[0]])
            s = (ctypes.c_float * 3)(*[float(v) for v in norm[1]])
        check(self.lib.uwie_resize_rgb_u8(self._ctx, _ptr(table), B, int(out_h), int(out_w), _ptr(f), _ptr(u8), _ptr(f32),
                                          _ptr(nrm), m, s, self.stream()))
        return u8, f32, nrm

    def quality_scores(self, frames_u8, frames_f32=None, weights=None, gray_shift: int = 15):
        """frames_u8: uint8 cuda [B,H,W,3] (the quantised image); frames_f32: optional float32 cuda [B,H,W,3];
        weights: optional 8 floats.  Returns float64 [B,9]: the eight scores (QUALITY_KEYS order) and the total."""
        B, H, W = self._bhw(frames_u8)
        assert frames_u8.dtype == torch.uint8
        if frames_f32 is not None:
            assert frames_f32.dtype == torch.float32 and tuple(frames_f32.shape) == (B, H, W, 3)
            frames_f32 = frames_f32.contiguous()
        ws = self.workspace_for(B, H, W)
        out = self.empty((B, 9), torch.float64)
        w = (ctypes.c_double * 8)(*[float(x) for x in weights]) if weights is not None else None
        check(self.lib.uwie_quality_scores(self._ctx, _ptr(frames_u8), _ptr(frames_f32), B, H, W, int(gray_shift), w,
                                           _ptr(out), _ptr(ws), ws.numel(), self.stream()))
        return out

    def select_best_u8(self, frames, plist, weights=None, want_all: bool = False):
        """main.py:118-146 on the device (uwie_select_best_u8): frames uint8 cuda [B,H,W,3], plist a list of UwieParams.
        Returns (best index int32 [B], best image uint8 [B,H,W,3], scores float64 [n,B,9], all outputs [n,B,H,W,3] or None)."""
        B, H, W = self._bhw(frames)
        assert frames.dtype == torch.uint8
        n = len(plist)
        arr = (UwieParams * n)(*plist)
        nbytes = self.lib.uwie_workspace_bytes_select(B, H, W, arr, n, int(want_all))
        if nbytes == 0:
            raise _lib.UwieError("select_best: batch/H/W or strategy count out of range")
        ws = self.workspace(nbytes)
        best = self.empty((B,), torch.int32)
        img = self.empty((B, H, W, 3), torch.uint8)
        scores = self.empty((n, B, 9), torch.float64)
        every = self.empty((n, B, H, W, 3), torch.uint8) if want_all else None
        w = (ctypes.c_double * 8)(*[float(x) for x in weights]) if weights is not None else None
        check(self.lib.uwie_select_best_u8(self._ctx, _ptr(frames), B, H, W, arr, n, w, _ptr(img), _ptr(best), _ptr(scores),
                                           _ptr(every), _ptr(ws), ws.numel(), self.stream()))
        return best, img, scores, every

    def underwater_scores(self, frames_u8, gray_shift: int = 15):
        """UCIQE / UIQM and their parts (uwie_underwater_scores_u8): frames uint8 cuda [B,H,W,3] -> float64 [B,8] in
        include/uwie.h's order (sigma_c, con_l, mu_s, UCIQE, UICM, UISM, UIConM, UIQM)."""
        B, H, W = self._bhw(frames_u8)
        assert frames_u8.dtype == torch.uint8
        ws = self._sized_workspace(self.lib.uwie_workspace_bytes_underwater(B, H, W), "underwater_scores: batch/H/W out of range")
        out = self.empty((B, _lib.UW_SCORES), torch.float64)
        check(self.lib.uwie_underwater_scores_u8(self._ctx, _ptr(frames_u8), B, H, W, int(gray_shift), _ptr(out), _ptr(ws),
                                                 ws.numel(), self.stream()))
        return out

    def reference_scores(self, frames_u8, refs_u8, gray_shift: int = 15):
        """MAE, MSE, PSNR and SSIM against a reference (uwie_reference_scores_u8): frames uint8 cuda [B,H,W,3], refs uint8 cuda
        [R,H,W,3] with R dividing B (frame i is compared with reference i % R) -> float64 [B,8] in include/uwie.h's order
        (mae, mse, psnr, ssim_y, ssim_r, ssim_g, ssim_b, ssim_rgb)."""
        B, H, W = self._bhw(frames_u8)
        R = int(refs_u8.shape[0])
        assert frames_u8.dtype == torch.uint8 and refs_u8.dtype == torch.uint8 and refs_u8.is_contiguous()
        if tuple(refs_u8.shape[1:]) != (H, W, 3):
            raise ValueError(f"reference_scores: references are {tuple(refs_u8.shape[1:])}, frames {(H, W, 3)}")
        if R < 1 or B % R:
            raise ValueError(f"reference_scores: {R} references do not divide {B} frames")
        ws = self._sized_workspace(self.lib.uwie_workspace_bytes_reference(B, H, W), "reference_scores: batch/H/W out of range")
        out = self.empty((B, _lib.REF_SCORES), torch.float64)
        check(self.lib.uwie_reference_scores_u8(self._ctx, _ptr(frames_u8), _ptr(refs_u8), B, R, H, W, int(gray_shift), _ptr(out),
                                                _ptr(ws), ws.numel(), self.stream()))
        return out

    def gray_world(self, frames_u8, red: float = 1.0, blue: float = 0.0, max_gain: float = 0.0, want_out: bool = True,
                   want_stats: bool = False, out=None):
        """Gray-world white balance with red-channel compensation (uwie_gray_world_u8): frames uint8 cuda [B,H,W,3] ->
        (balanced uint8 [B,H,W,3] or None, stats float64 [B,12] in include/uwie.h's order or None).  ``out``: where the bytes go
        (``frames_u8`` itself for in place; default a new tensor); without ``want_out`` and ``out`` only the stats are computed."""
        B, H, W = self._bhw(frames_u8)
        assert frames_u8.dtype == torch.uint8
        if out is not None:
            assert out.dtype == torch.uint8 and tuple(out.shape) == (B, H, W, 3) and out.is_contiguous()
        elif want_out:
            out = self.empty((B, H, W, 3), torch.uint8)
        if out is None and not want_stats:
            raise ValueError("gray_world: nothing asked for (want_out, want_stats or out)")
        ws = self._sized_workspace(self.lib.uwie_workspace_bytes_gray_world(B, H, W), "gray_world: batch/H/W out of range")
        stats = self.empty((B, _lib.GW_STATS), torch.float64) if want_stats else None
        check(self.lib.uwie_gray_world_u8(self._ctx, _ptr(frames_u8), B, H, W, float(red), float(blue), float(max_gain), _ptr(out),
                                          _ptr(stats), _ptr(ws), ws.numel(), self.stream()))
        return out, stats

    def fusion(self, frames_u8, gamma: float = 2.2, levels: int = 1, gray_shift: int = 15, want_parts: bool = False):
        """Multi-scale fusion of a gamma-corrected and a sharpened input (uwie_fusion_u8): balanced frames uint8 cuda [B,H,W,3]
        -> (fused uint8 [B,H,W,3], parts); parts is None, or with ``want_parts`` (in1 uint8 [B,H,W,3], in2 uint8 [B,H,W,3],
        weight float64 [B,H,W] = the normalised weight of input 1)."""
        B, H, W = self._bhw(frames_u8)
        assert frames_u8.dtype == torch.uint8
        ws = self._sized_workspace(self.lib.uwie_workspace_bytes_fusion(B, H, W, int(levels)), "fusion: batch/H/W/levels out of range")
        out = self.empty((B, H, W, 3), torch.uint8)
        parts = None
        if want_parts:
            parts = (self.empty((B, H, W, 3), torch.uint8), self.empty((B, H, W, 3), torch.uint8), self.empty((B, H, W), torch.float64))
        in1, in2, weight = parts if parts else (None, None, None)
        check(self.lib.uwie_fusion_u8(self._ctx, _ptr(frames_u8), B, H, W, float(gamma), int(levels), int(gray_shift), _ptr(out), _ptr(in1),
                                      _ptr(in2), _ptr(weight), _ptr(ws), ws.numel(), self.stream()))
        return out, parts

    def pick_best_u8(self, scores, col: int, every=None):
        """uwie_pick_best_u8: scores float64 cuda [n,B,ncols] -> (first argmax over the sets of column ``col`` as int32 [B],
        the winners' frames [B,H,W,3] gathered from ``every`` [n,B,H,W,3], or None without it)."""
        assert scores.dtype == torch.float64 and scores.dim() == 3 and scores.is_contiguous()
        n, B, ncols = (int(v) for v in scores.shape)
        best = self.empty((B,), torch.int32)
        img, H, W = None, 0, 0
        if every is not None:
            assert every.dtype == torch.uint8 and every.is_contiguous() and every.dim() == 5 and tuple(every.shape[:2]) == (n, B)
            H, W = int(every.shape[2]), int(every.shape[3])
            img = self.empty((B, H, W, 3), torch.uint8)
        check(self.lib.uwie_pick_best_u8(self._ctx, _ptr(scores), n, B, ncols, int(col), _ptr(every), H, W, _ptr(best), _ptr(img),
                                         self.stream()))
        return best, img

    # ------------------------------------------------------------------ stages
    def cast_classify(self, frames):
        B, H, W = self._bhw(frames)
        ws = self.workspace_for(B, H, W)
        kind = self.empty((B,), torch.int32)
        mean = self.empty((B, 3), torch.float32)
        check(self.lib.uwie_cast_classify(self._ctx, _ptr(frames), B, H, W, _ptr(kind), _ptr(mean), _ptr(ws),
                                          ws.numel(), self.stream()))
        return kind, mean

    def normalise_correct(self, frames, kind=None):
        B, H, W = self._bhw(frames)
        out = self.empty((B, H, W, 3), torch.float32)
        check(self.lib.uwie_normalise_correct(self._ctx, _ptr(frames), _ptr(kind), _ptr(out), B, H, W, self.stream()))
        return out

    def atmospheric_light(self, frames, kind=None, p: UwieParams | None = None, trace: bool = False, want_gray: bool = False):
        """``want_gray``: also return the gray plane the call wrote on its way (uwie_atmospheric_light keeps it in the first
        B*H*W bytes of its workspace) -- tests compare it with ``transmission_init``'s."""
        B, H, W = self._bhw(frames)
        p = p or self.params(_lib.SURFACE_SIX, 2)
        ws = self.workspace_for(B, H, W, p)
        A = self.empty((B, 3), torch.float32)
        tr = torch.zeros((B, 32, _TRACE_DTYPE.itemsize), dtype=torch.uint8, device=self.torch_device) if trace else None
        check(self.lib.uwie_atmospheric_light(self._ctx, _ptr(frames), _ptr(kind), B, H, W, ctypes.byref(p), _ptr(A),
                                              _ptr(tr), _ptr(ws), ws.numel(), self.stream()))
        out = (A, tr.cpu().numpy().view(_TRACE_DTYPE).reshape(B, 32)) if trace else A
        if want_gray:
            gray = ws[: B * H * W].view(B, H, W).clone()
            return (*out, gray) if trace else (out, gray)
        return out

    def transmission_init(self, frames, A, kind=None, p: UwieParams | None = None):
        B, H, W = self._bhw(frames)
        p = p or self.params(_lib.SURFACE_SIX, 2)
        t0 = self.empty((B, H, W), torch.float32)
        gray = self.empty((B, H, W), torch.uint8)
        check(self.lib.uwie_transmission_init(self._ctx, _ptr(frames), _ptr(kind), _ptr(A), B, H, W, ctypes.byref(p),
                                              _ptr(t0), _ptr(gray), self.stream()))
        return t0, gray

    def box_filter_f64(self, planes, ksize):
        B, H, W = (int(v) for v in planes.shape)
        assert planes.dtype == torch.float64 and planes.is_contiguous()
        ws = self.workspace_for(B, H, W)
        out = torch.empty_like(planes)
        check(self.lib.uwie_box_filter_f64(self._ctx, _ptr(planes), _ptr(out), B, H, W, int(ksize), _ptr(ws), ws.numel(),
                                           self.stream()))
        return out

    def guided_filter(self, gray, t0, ksize, eps, exact=True):
        B, H, W = (int(v) for v in gray.shape)
        ws = self.workspace_for(B, H, W)
        t = self.empty((B, H, W), torch.float64)
        check(self.lib.uwie_guided_filter(self._ctx, _ptr(gray), _ptr(t0), B, H, W, int(ksize), float(eps), int(exact), _ptr(t),
                                          _ptr(ws), ws.numel(), self.stream()))
        return t

    def restore(self, frames, A, t, kind=None):
        B, H, W = self._bhw(frames)
        out = self.empty((B, H, W, 3), torch.float32)
        check(self.lib.uwie_restore(self._ctx, _ptr(frames), _ptr(kind), _ptr(A), _ptr(t), B, H, W, _ptr(out),
                                    self.stream()))
        return out

    def percentiles_f32(self, img, q_percent):
        B, H, W = self._bhw(img)
        assert img.dtype == torch.float32
        q = (ctypes.c_double * len(q_percent))(*[float(v) for v in q_percent])
        ws = self.workspace_for(B, H, W)
        out = self.empty((B, 3, len(q_percent)), torch.float32)
        check(self.lib.uwie_percentiles_f32(self._ctx, _ptr(img), B, H, W, q, len(q_percent), _ptr(out), _ptr(ws),
                                            ws.numel(), self.stream()))
        return out

    def percentiles_f64(self, img, q_percent):
        B, H, W = self._bhw(img)
        assert img.dtype == torch.float64
        q = (ctypes.c_double * len(q_percent))(*[float(v) for v in q_percent])
        ws = self.workspace_for(B, H, W)
        out = self.empty((B, 3, len(q_percent)), torch.float64)
        check(self.lib.uwie_percentiles_f64(self._ctx, _ptr(img), B, H, W, q, len(q_percent), _ptr(out), _ptr(ws),
                                            ws.numel(), self.stream()))
        return out

    def stretch_f32(self, img, lo, hi):
        B, H, W = self._bhw(img)
        ws = self.workspace_for(B, H, W)
        out = torch.empty_like(img)
        check(self.lib.uwie_stretch_f32(self._ctx, _ptr(img), _ptr(out), B, H, W, float(lo), float(hi), _ptr(ws),
                                        ws.numel(), self.stream()))
        return out

    def gamma_f32(self, img, g, mode=1):
        out = torch.empty_like(img)
        check(self.lib.uwie_gamma_f32(self._ctx, _ptr(img), _ptr(out), img.numel(), float(g), int(mode), self.stream()))
        return out

    def _clahe_workspace(self, B, H, W, tiles):
        """A workspace sized for the tile LUTs of this grid (the default parameter set answers for 8 x 8)."""
        return self.workspace_for(B, H, W, self.params(_lib.SURFACE_SIX, 2, tiles_x=int(tiles[0]), tiles_y=int(tiles[1])))

    def clahe_f32(self, img, clip, tiles=(8, 8)):
        B, H, W = self._bhw(img)
        ws = self._clahe_workspace(B, H, W, tiles)
        out = torch.empty_like(img)
        check(self.lib.uwie_clahe_f32(self._ctx, _ptr(img), _ptr(out), B, H, W, float(clip), int(tiles[0]),
                                      int(tiles[1]), _ptr(ws), ws.numel(), self.stream()))
        return out

    def rgb2gray_u8(self, rgb, gray_shift=15):
        out = self.empty(rgb.shape[:-1], torch.uint8)
        check(self.lib.uwie_rgb2gray_u8(self._ctx, _ptr(rgb), _ptr(out), out.numel(), int(gray_shift), self.stream()))
        return out

    def rgb2lab_u8(self, rgb):
        out = torch.empty_like(rgb)
        check(self.lib.uwie_rgb2lab_u8(self._ctx, _ptr(rgb), _ptr(out), rgb.numel() // 3, self.stream()))
        return out

    def lab2rgb_u8(self, lab):
        out = torch.empty_like(lab)
        check(self.lib.uwie_lab2rgb_u8(self._ctx, _ptr(lab), _ptr(out), lab.numel() // 3, self.stream()))
        return out

    def clahe_u8(self, planes, clip, tiles=(8, 8)):
        B, H, W = (int(v) for v in planes.shape)
        ws = self._clahe_workspace(B, H, W, tiles)
        out = torch.empty_like(planes)
        check(self.lib.uwie_clahe_u8(self._ctx, _ptr(planes), _ptr(out), B, H, W, float(clip), int(tiles[0]),
                                     int(tiles[1]), _ptr(ws), ws.numel(), self.stream()))
        return out

    def canny_u8(self, gray, low=50, high=150):
        B, H, W = (int(v) for v in gray.shape)
        ws = self.workspace_for(B, H, W)
        out = torch.empty_like(gray)
        check(self.lib.uwie_canny_u8(self._ctx, _ptr(gray), _ptr(out), B, H, W, int(low), int(high), _ptr(ws),
                                     ws.numel(), self.stream()))
        return out

    def equalize_hist_u8(self, planes):
        B, H, W = (int(v) for v in planes.shape)
        ws = self.workspace_for(B, H, W)
        out = torch.empty_like(planes)
        check(self.lib.uwie_equalize_hist_u8(self._ctx, _ptr(planes), _ptr(out), B, H, W, _ptr(ws), ws.numel(),
                                             self.stream()))
        return out


class HandleOwner(_ClosedOnDel):
    """What owns device handles of frozen weights (uwie_vgg, uwie_param_net, uwie_mlp, uwie_mlp_trainer, uwie_model): one per
    key -- the GPU, then whatever else ``_handle`` is given -- made at first use and freed by ``close()``, which ``__del__``
    runs too.  A subclass says how: ``_create_handle(dev, *key)`` and ``_destroy_handle(dev, handle)``.  Both synchronise
    the GPU.  After ``close()`` the next use creates again."""

    def _handle(self, dev: Device, *key):
        handles = self.__dict__.setdefault("_handles", {})  # (GPU index, *key) -> (dev, handle)
        at = (dev.index,) + key
        if at not in handles:
            handles[at] = dev, self._create_handle(dev, *key)
        return handles[at][1]

    def close(self):
        handles = self.__dict__.get("_handles", {})
        while handles:
            dev, handle = handles.popitem()[1]
            self._destroy_handle(dev, handle)


_devices: dict[int, Device] = {}


def get_device(index: int | None = None) -> Device:
    if index is None:
        index = torch.cuda.current_device() if torch.cuda.is_available() else 0
    if index not in _devices:
        _devices[index] = Device(index)
    return _devices[index]
