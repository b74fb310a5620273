"""The training-side surfaces: the two ``DifferentiableEnhancement`` modules with their autograd Functions, and
``ReferenceLoss`` with the loss fused into the modules' sweeps (DESIGN.md sections 8, 10 and 13).

Both modules share one host path: one image check (``_image_batch``), one builder of the device's ``[B,4]`` parameter
columns (``_param_columns``), one fused-loss step (``_module_loss``).  A module class states what differs: its keys, its
autograd Functions, and whether a call polls the device for an unindexable sorted position.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib
from .runtime import Device, get_device


def _image_batch(dev: Device, img):
    """The image batch of a module call: float32 ``(B, 3, H, W)`` on ``dev`` from a torch tensor or a NumPy array (float64
    NumPy input is converted; ValueError otherwise)."""
    x = img.to(dev.torch_device) if isinstance(img, torch.Tensor) else dev.tensor(np.ascontiguousarray(img, dtype=np.float32))
    if x.dtype != torch.float32:
        raise ValueError(f"expected a float32 image batch, got {x.dtype}")
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"expected a (B, 3, H, W) image batch, got {tuple(x.shape)}")
    return x


def _param_columns(dev: Device, params, spec, B: int, grad: bool):
    """A module's dict of ``(B, 1)``-shaped values -> ``(pt, flags)``: ``pt`` float32 ``[B,4]`` contiguous on ``dev`` in
    ``spec``'s order, ``flags`` with bit ``i - 2`` set when the optional key ``i`` is present.  ``spec`` is ``((key, default
    or None), ...)``: a missing key takes its default (its stage is skipped), one without a default raises ``KeyError``.
    The first two columns are the sorted positions, which never carry a gradient (the references read them with
    ``.item()``); the others carry one only when ``grad``."""
    cols, flags = [], 0
    for i, (key, default) in enumerate(spec):
        if key in params:
            v = params[key]
            v = (v.to(device=dev.torch_device, dtype=torch.float32) if isinstance(v, torch.Tensor)
                 else torch.as_tensor(np.asarray(v, dtype=np.float32), device=dev.torch_device))
            if i < 2 or not grad:
                v = v.detach()
            cols.append(torch.broadcast_to(v.reshape(-1), (B,)))
            if default is not None:
                flags |= 1 << (i - 2)
        elif default is None:
            raise KeyError(key)
        else:
            cols.append(torch.full((B,), default, dtype=torch.float32, device=dev.torch_device))
    return torch.stack(cols, dim=1).contiguous(), flags


def _raise_rank_error(L, n: int):
    """Raise what ``color_stretch`` (deep_learning_parameters.py:73-77) raises first for ``L`` float32 ``[B,2]``: per image
    ``int(L_low / 100.0 * n)``, ``int(L_high / 100.0 * n)`` (ValueError for NaN, OverflowError for inf), then the two
    indexings (IndexError outside ``[-n, n - 1]``, ValueError beyond int64: torch's messages)."""
    for lo, hi in np.asarray(L, dtype=np.float32).reshape(-1, 2):
        ks = [int(float(v) / 100.0 * n) for v in (lo, hi)]
        for k in ks:
            if not -2**63 <= k < 2**63:
                raise ValueError("Overflow when unpacking long long")
            if not -n <= k < n:
                raise IndexError(f"index {k} is out of bounds for dimension 0 with size {n}")


def _raise_flagged_rank(x, pt):
    """The device flagged a sorted position of ``pt`` for the planes of ``x``: raise the reference's exception for it."""
    _raise_rank_error(pt[:, :2].detach().cpu().numpy(), x.shape[2] * x.shape[3])
    raise _lib.UwieError("diff_gated: the device flagged a sorted position that the host finds valid")


# ------------------------------------------------------------------ the autograd Functions of the two modules
class _ModuleFunction(torch.autograd.Function):
    """A module's device forward with its backward: the shared body of ``DiffEnhanceFunction`` (MAP = LOSS_VGG, whose Device
    methods take ``flags``) and ``GatedDiffEnhanceFunction`` (LOSS_GATED, whose methods take none)."""

    MAP = None

    @classmethod
    def _run(cls, ctx, img, params, flags, planar, dev):
        if cls.MAP == _lib.LOSS_VGG:
            out, saved = dev.diff_enhance_save_f32(img, params, planar, flags)
        else:
            out, saved = dev.diff_gated_save_f32(img, params, planar)
        ctx.save_for_backward(img, params, saved)
        ctx.flags, ctx.planar, ctx.dev = flags, planar, dev
        return out

    @classmethod
    def _grad(cls, ctx, grad_out):
        img, params, saved = ctx.saved_tensors
        grad_out, want_img = grad_out.float().contiguous(), ctx.needs_input_grad[0]
        if cls.MAP == _lib.LOSS_VGG:
            grad_img, grad_params = ctx.dev.diff_enhance_bwd_f32(img, params, saved, grad_out, ctx.planar, ctx.flags,
                                                                 want_img=want_img)
        else:
            grad_img, grad_params = ctx.dev.diff_gated_bwd_f32(img, params, saved, grad_out, ctx.planar, want_img=want_img)
        return grad_img, (grad_params if ctx.needs_input_grad[1] else None)


class DiffEnhanceFunction(_ModuleFunction):
    """``out = DiffEnhanceFunction.apply(img, params, flags, planar, dev)``: the device forward with its backward.

    ``img``: float32 ``[B,3,H,W]`` (planar) or ``[B,H,W,3]`` on ``dev``; ``params``: float32 ``[B,4]`` =
    ``L_low, L_high, omega, gamma``; ``flags``: ``UWIE_DIFF_OMEGA (1) | UWIE_DIFF_GAMMA (2)``.  The gradient is the one
    torch autograd gives the reference module on the CPU: ``params`` gets ``0, 0, d omega,
    d gamma``; ``img`` gets its gradient only when it requires one (otherwise the kernel skips that write).
    """

    MAP = _lib.LOSS_VGG

    @staticmethod
    def forward(ctx, img, params, flags, planar, dev):
        return DiffEnhanceFunction._run(ctx, img, params, flags, planar, dev)

    @staticmethod
    def backward(ctx, grad_out):
        return DiffEnhanceFunction._grad(ctx, grad_out) + (None, None, None)


class GatedDiffEnhanceFunction(_ModuleFunction):
    """``out = GatedDiffEnhanceFunction.apply(img, params, planar, dev)``: the gated module's device forward with its backward.

    ``img``: float32 ``[B,3,H,W]`` (planar) or ``[B,H,W,3]`` on ``dev``; ``params``: float32 ``[B,4]`` =
    ``L_low, L_high, use_gamma, gamma``.  The gradient is the one torch autograd gives the reference module on the CPU
    (DESIGN.md section 10): ``params`` gets ``0, 0, d use_gamma, d gamma``; ``img`` gets its gradient only when it requires
    one.  An image without a valid sorted position gets NaN and sets UWIE_STATUS_DIFF_RANK: this function does not check
    it (``GatedDifferentiableEnhancement`` does).
    """

    MAP = _lib.LOSS_GATED

    @staticmethod
    def forward(ctx, img, params, planar, dev):
        return GatedDiffEnhanceFunction._run(ctx, img, params, 0, planar, dev)

    @staticmethod
    def backward(ctx, grad_out):
        return GatedDiffEnhanceFunction._grad(ctx, grad_out) + (None, None)


# ------------------------------------------------------------------ ReferenceLoss's Functions (deep_learning_parameters.py:170-196, N9)
def _loss_backward(ctx, map_, img, params, saved, ref, grad_l1, grad_l2, grad_out=None):
    """The shared backward of the three loss functions: dL/dl1, dL/dl2 go to the kernel as a device [2] (zeros for an
    unused output), grad_out (dL/d(out), or None) as the upstream gradient of the kept output."""
    dev = ctx.dev
    z = None
    if grad_l1 is None or grad_l2 is None:
        z = torch.zeros((), dtype=torch.float32, device=dev.torch_device)
    gl = torch.stack([(z if grad_l1 is None else grad_l1).float().reshape(()),
                      (z if grad_l2 is None else grad_l2).float().reshape(())])
    return dev.ref_loss_bwd_f32(map_, img, params, saved, ref, gl, ctx.planar, ctx.flags,
                                grad_out=None if grad_out is None else grad_out.float(),
                                want_img=ctx.needs_input_grad[0])


class RefLossFunction(torch.autograd.Function):
    """``l1, l2 = RefLossFunction.apply(o, ref, dev, sink)``: ``mean|o - ref|`` and ``mean((o - ref)^2)`` on the device
    (uwie_ref_loss_f32, identity map), 0-dim float32.  ``o``, ``ref``: float32 ``(B, 3, H, W)`` on ``dev``.  The backward
    gives ``o`` the gradient torch CPU autograd gives it, bit for bit; ``ref`` gets none.  ``sink`` (a list or None)
    receives the device buffer whose first two words are l1, l2."""

    @staticmethod
    def forward(ctx, o, ref, dev, sink=None):
        _, _, buf = dev.ref_loss_f32(_lib.LOSS_IDENTITY, o, None, ref, True)
        ctx.save_for_backward(o, ref)
        ctx.dev, ctx.planar, ctx.flags = dev, True, 0
        ctx.set_materialize_grads(False)
        if sink is not None:
            sink.append(buf)
        return buf[0], buf[1]

    @staticmethod
    def backward(ctx, grad_l1, grad_l2):
        o, ref = ctx.saved_tensors
        if grad_l1 is None and grad_l2 is None:
            return None, None, None, None
        grad_o, _ = _loss_backward(ctx, _lib.LOSS_IDENTITY, o, None, None, ref, grad_l1, grad_l2)
        return grad_o, None, None, None


class _ModuleLossFunction(torch.autograd.Function):
    """The fused module step: ``[out,] l1, l2 = F.apply(img, params, ref, flags, planar, keep_out, status, dev, sink)``."""

    MAP = None

    @classmethod
    def _run(cls, ctx, img, params, ref, flags, planar, keep_out, status, dev, sink):
        out, saved, buf = dev.ref_loss_f32(cls.MAP, img, params, ref, planar, flags, want_out=keep_out, status=status)
        ctx.save_for_backward(img, params, saved, ref)
        ctx.dev, ctx.planar, ctx.flags, ctx.keep_out = dev, planar, flags, keep_out
        ctx.set_materialize_grads(False)
        if sink is not None:
            sink.append(buf)
        return (out, buf[0], buf[1]) if keep_out else (buf[0], buf[1])

    @classmethod
    def _grad(cls, ctx, grads):
        img, params, saved, ref = ctx.saved_tensors
        grad_out, grad_l1, grad_l2 = grads if ctx.keep_out else (None,) + tuple(grads)
        none = (None,) * 7
        if grad_out is None and grad_l1 is None and grad_l2 is None:
            return (None, None) + none
        grad_img, grad_params = _loss_backward(ctx, cls.MAP, img, params, saved, ref, grad_l1, grad_l2, grad_out)
        return (grad_img, grad_params if ctx.needs_input_grad[1] else None) + none


class DiffEnhanceLossFunction(_ModuleLossFunction):
    """``vgg_16_UIE.DifferentiableEnhancement`` with the loss fused in (uwie_ref_loss_f32, UWIE_LOSS_VGG): ``img``,
    ``params`` and ``flags`` as in ``DiffEnhanceFunction``, ``ref`` in ``img``'s layout.  Outputs ``(l1, l2)``, or
    ``(out, l1, l2)`` with ``keep_out``; gradients reach ``img`` and ``params`` as through ``DiffEnhanceFunction``."""

    MAP = _lib.LOSS_VGG

    @staticmethod
    def forward(ctx, img, params, ref, flags, planar, keep_out, status, dev, sink=None):
        return DiffEnhanceLossFunction._run(ctx, img, params, ref, flags, planar, keep_out, status, dev, sink)

    @staticmethod
    def backward(ctx, *grads):
        return DiffEnhanceLossFunction._grad(ctx, grads)


class GatedDiffEnhanceLossFunction(_ModuleLossFunction):
    """``deep_learning_parameters.DifferentiableEnhancement`` with the loss fused in (UWIE_LOSS_GATED): as
    ``GatedDiffEnhanceFunction`` (``flags`` 0), outputs as ``DiffEnhanceLossFunction``.  An image without a valid sorted
    position makes l1, l2 NaN and sets UWIE_STATUS_DIFF_RANK; this function does not check it."""

    MAP = _lib.LOSS_GATED

    @staticmethod
    def forward(ctx, img, params, ref, flags, planar, keep_out, status, dev, sink=None):
        return GatedDiffEnhanceLossFunction._run(ctx, img, params, ref, flags, planar, keep_out, status, dev, sink)

    @staticmethod
    def backward(ctx, *grads):
        return GatedDiffEnhanceLossFunction._grad(ctx, grads)


def _frames_u8(module, frames_u8, out: str):
    """The common front of the modules' ``enhance_u8``: (dev, uint8 [B,H,W,3] on it, was_numpy, single)."""
    if out not in ("u8", "float32"):
        raise ValueError(f"out is 'u8' or 'float32', got {out!r}")
    dev = get_device(module.device)
    was_numpy = not isinstance(frames_u8, torch.Tensor)
    t = torch.from_numpy(np.ascontiguousarray(frames_u8)) if was_numpy else frames_u8
    if t.dtype != torch.uint8:
        raise TypeError(f"expected uint8 frames, got {t.dtype}")
    single = t.dim() == 3
    if single:
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[-1] != 3 or t.numel() == 0:
        raise ValueError(f"expected non-empty [H,W,3] or [B,H,W,3] frames, got {tuple(frames_u8.shape)}")
    return dev, t.to(dev.torch_device).contiguous(), was_numpy, single


def _finish_u8(res, was_numpy, single):
    if single:
        res = res[0]
    return res.cpu().numpy() if was_numpy else res


# ------------------------------------------------------------------ the two modules
class _EnhancementModule:
    """What the two modules share.  A subclass states ``_SPEC`` (its keys in the device's column order, each with its
    default or None when required), ``_FUNCTION`` / ``_LOSS_FUNCTION`` (its autograd Functions, whose ``MAP`` is its
    ``_lib.LOSS_*``) and ``_POLLS_RANK`` (a call waits for the device once and raises the reference's exception for an
    unindexable sorted position), and runs its own forward in ``_run``."""

    device: int | None = None
    _SPEC = ()
    _FUNCTION = _LOSS_FUNCTION = None
    _POLLS_RANK = False

    def _begin(self, img, params):
        """(dev, the image batch on it): the first errors of a call, in the reference's order."""
        dev = get_device(self.device)
        return dev, _image_batch(dev, img)

    def _columns(self, dev: Device, x, params):
        """(pt, flags, grad): the parameter columns for the image batch ``x``, and whether this call carries a graph."""
        grad = torch.is_grad_enabled() and any(isinstance(v, torch.Tensor) and v.requires_grad
                                               for v in [x] + [params[k] for k, _ in self._SPEC if k in params])
        pt, flags = _param_columns(dev, params, self._SPEC, x.shape[0], grad)
        return pt, flags, grad

    def forward(self, img, params):
        dev, x = self._begin(img, params)
        pt, flags, grad = self._columns(dev, x, params)
        out = self._run(dev, x, pt, flags, grad)
        if self._POLLS_RANK and dev.check_status(allow=_lib.STATUS_DIFF_RANK) & _lib.STATUS_DIFF_RANK:
            _raise_flagged_rank(x, pt)
        return out if grad or isinstance(img, torch.Tensor) else out.cpu().numpy()

    __call__ = forward

    def with_loss(self, images, params, references):
        """``(out, l1, l2)``: the module's output (the inference forward's bytes) with ``l1 = mean|out - references|`` and
        ``l2 = mean((out - references)^2)`` from the same sweep (ReferenceLoss).  With grad mode on,
        ``out``, ``l1`` and ``l2`` all carry the graph: a term of the caller's on ``out`` (CombinedLoss's perceptual loss)
        adds its gradient in the same backward.  ``references``: float32, ``images``' shape (ValueError otherwise).
        The gated module waits once per call, as its forward does, and raises what forward raises for an unindexable
        sorted position; the vgg module does not wait."""
        sink = []
        dev, (out, l1, l2), x, pt = _module_loss(self, images, params, references, True, self._POLLS_RANK, sink)
        if self._POLLS_RANK:
            _read_loss(dev, sink[0], x, pt)
        return out, l1, l2


class DifferentiableEnhancement(_EnhancementModule):
    """``vgg_16_UIE.DifferentiableEnhancement`` (vgg_16_UIE.py:24-128) on the device, forward and backward.

    ``forward(img, params)``: ``img`` is ``(B, 3, H, W)`` float32 (NumPy or torch tensor), ``params`` a dict of
    ``(B, 1)``-shaped values with the reference's keys: ``L_low`` and ``L_high`` are required, ``omega`` and ``gamma``
    optional (a missing key skips that stage, vgg_16_UIE.py:48,52).

    Differentiable: with grad mode on and ``img`` or a parameter tensor requiring grad, the output carries a ``grad_fn``
    and ``loss.backward()`` runs the gradient kernels (``DiffEnhanceFunction``).  ``omega`` and ``gamma`` get the
    gradient torch autograd gives the reference on the CPU, in their own dtype and device (float16 / bfloat16 values
    from an autocast head are cast to float32 first, as torch's type promotion does in the reference); ``L_low`` and
    ``L_high`` get none (the reference reads them with ``.item()``); ``img`` gets one when it requires it.  Otherwise
    the forward alone runs, as for inference.
    """

    _SPEC = (("L_low", None), ("L_high", None), ("omega", 0.0), ("gamma", 1.0))
    _FUNCTION, _LOSS_FUNCTION = DiffEnhanceFunction, DiffEnhanceLossFunction

    def _run(self, dev: Device, x, pt, flags, grad):
        if grad:
            return self._FUNCTION.apply(x, pt, flags, True, dev)
        return dev.diff_enhance_f32(x, pt, planar=True, has_omega=bool(flags & 1), has_gamma=bool(flags & 2))

    def enhance_image(self, img, params):
        """``EnhancementPredictor.enhance_image(img, params)`` (use_trained_model.py:83-111) with explicit parameters:
        ``img`` HxWx3 RGB float in [0, 1], ``params`` a dict of Python floats with ``omega, gamma, L_low, L_high``."""
        dev = get_device(self.device)
        x = np.ascontiguousarray(np.asarray(img, dtype=np.float32))
        if x.ndim != 3 or x.shape[2] != 3:
            raise ValueError(f"expected an HxWx3 image, got {x.shape}")
        pt = dev.tensor(np.array([[params["L_low"], params["L_high"], params["omega"], params["gamma"]]], np.float32))
        out = dev.diff_enhance_f32(dev.tensor(x[None]), pt, planar=False)[0].cpu().numpy()
        return np.clip(out, 0.0, 1.0)

    def enhance_u8(self, frames_u8, params, out: str = "u8"):
        """The forward for uint8 frames in the byte domain (uwie_diff_enhance_u8): inference only, no
        autograd.  ``frames_u8``: ``[H,W,3]`` / ``[B,H,W,3]`` uint8, NumPy (the result comes back as NumPy) or a torch tensor
        (it stays on the device); the image is ``u8 / 255``.  ``params``: the module's dict, as for ``forward``.
        ``out="float32"``: the module's output in the frames' layout, the bits ``forward`` gives for ``u8 / 255``;
        ``out="u8"``: ``(np.clip(that, 0, 1) * 255).astype(np.uint8)``, use_trained_model.py:131."""
        dev, t, was_numpy, single = _frames_u8(self, frames_u8, out)
        pt, flags = _param_columns(dev, params, self._SPEC, t.shape[0], False)
        o8, o32 = dev.diff_enhance_u8(t, pt, flags, want_u8=out == "u8", want_f32=out == "float32")
        return _finish_u8(o8 if out == "u8" else o32, was_numpy, single)


class GatedDifferentiableEnhancement(_EnhancementModule):
    """``deep_learning_parameters.DifferentiableEnhancement`` (deep_learning_parameters.py:24-90) on the device, forward and
    backward: the module ``EndToEndTrainer`` trains through.

    ``forward(img, params)``: ``img`` is ``(B, 3, H, W)`` float32 (NumPy or torch tensor), ``params`` a dict of
    ``(B, 1)``-shaped values with all four of the reference's keys, ``L_low``, ``L_high``, ``use_gamma`` and ``gamma`` (a
    missing one raises ``KeyError``).  Per plane: stretch between the sorted positions ``int(L / 100.0 * n)`` (Python's
    indexing rules, no clamp), then ``clamp(use_gamma * pow(s + 1e-8, 1.0 / gamma) + (1 - use_gamma) * s, 0, 1)``.

    Differentiable: with grad mode on and ``img`` or a parameter tensor requiring grad, the output carries a ``grad_fn``
    and ``loss.backward()`` runs the gradient kernels (``GatedDiffEnhanceFunction``).  ``use_gamma`` and ``gamma`` get the
    gradient torch autograd gives the reference on the CPU, in their own dtype and device; ``L_low`` and ``L_high`` get none
    (the reference reads them with ``.item()``); ``img`` gets one when it requires it.  Otherwise the forward alone runs,
    with the same output bytes.

    Errors: each call waits for the device once, after the forward.  A sorted position the reference could not index raises
    the exception the reference raises there: ``IndexError`` (outside ``[-n, n - 1]``), ``ValueError`` (NaN ``L``, or a
    position beyond int64), ``OverflowError`` (infinite ``L``).  Every other device status bit still raises ``UwieError``.
    """

    KEYS = ("L_low", "L_high", "use_gamma", "gamma")
    _SPEC = tuple((k, None) for k in KEYS)
    _FUNCTION, _LOSS_FUNCTION = GatedDiffEnhanceFunction, GatedDiffEnhanceLossFunction
    _POLLS_RANK = True

    def _begin(self, img, params):
        for k in self.KEYS:
            params[k]  # KeyError in the reference's order, before the image is looked at
        return super()._begin(img, params)

    def _run(self, dev: Device, x, pt, flags, grad):
        if grad:
            return self._FUNCTION.apply(x, pt, True, dev)
        return dev.diff_gated_f32(x, pt, planar=True)

    def enhance_u8(self, frames_u8, params, out: str = "u8"):
        """The forward for uint8 frames in the byte domain (uwie_diff_gated_u8): inference only, no
        autograd.  Arguments and results as ``DifferentiableEnhancement.enhance_u8``; ``params`` needs all four keys.  Per
        image the module is a 3 x 256 table of the byte, so ``out="float32"`` gives the bits ``forward`` gives for
        ``u8 / 255`` and ``out="u8"`` their ``(x * 255).astype(np.uint8)``.  One wait per call; an unindexable sorted position
        raises what ``forward`` raises."""
        for k in self.KEYS:
            params[k]
        dev, t, was_numpy, single = _frames_u8(self, frames_u8, out)
        pt, _ = _param_columns(dev, params, self._SPEC, t.shape[0], False)
        o8, o32 = dev.diff_gated_u8(t, pt, want_u8=out == "u8", want_f32=out == "float32")
        if self._POLLS_RANK and dev.check_status(allow=_lib.STATUS_DIFF_RANK) & _lib.STATUS_DIFF_RANK:
            _raise_rank_error(pt[:, :2].cpu().numpy(), t.shape[1] * t.shape[2])
            raise _lib.UwieError("diff_gated_u8: the device flagged a sorted position that the host finds valid")
        return _finish_u8(o8 if out == "u8" else o32, was_numpy, single)


# ------------------------------------------------------------------ ReferenceLoss (deep_learning_parameters.py:170-196, N9)
def _loss_reference(dev: Device, x, references):
    """The reference batch of a fused call: float32, x's shape, on x's device (ValueError otherwise)."""
    if not isinstance(references, torch.Tensor):
        references = np.asarray(references)
        if references.dtype != np.float32:
            raise ValueError(f"expected a float32 reference batch, got {references.dtype}")
        references = dev.tensor(np.ascontiguousarray(references))
    if references.dtype != torch.float32:
        raise ValueError(f"expected a float32 reference batch, got {references.dtype}")
    if tuple(references.shape) != tuple(x.shape):
        raise ValueError(f"the reference batch {tuple(references.shape)} does not match the image batch {tuple(x.shape)}")
    return references.to(dev.torch_device).contiguous()


def _module_loss(module, images, params, references, keep_out: bool, status: bool, sink):
    """The fused step for either module class: (dev, outputs of its loss Function, the image batch, the parameter columns
    ``_read_loss`` needs to explain a flagged sorted position: None for a module that flags none)."""
    if not isinstance(module, _EnhancementModule):
        raise TypeError(f"expected a DifferentiableEnhancement or GatedDifferentiableEnhancement, got {type(module).__name__}")
    dev, x = module._begin(images, params)
    try:
        ref = _loss_reference(dev, x, references)
    except ValueError:
        if module._POLLS_RANK:
            with torch.no_grad():
                module(x, params)  # the module's own errors (an unindexable position) come first, as in the reference
        raise
    pt, flags, _ = module._columns(dev, x, params)
    res = module._LOSS_FUNCTION.apply(x, pt, ref, flags, True, keep_out, status, dev, sink)
    return dev, res, x, (pt if module._POLLS_RANK else None)


def _read_loss(dev: Device, buf, x=None, pt=None, extra=None):
    """The one host read of a fused call: buf = {l1, l2, status bits} -> (l1, l2) as Python floats.  A flagged sorted position
    raises the reference's exception (first), any other status bit UwieError.  ``extra`` (a device float32 [1], e.g. the
    perceptual loss) comes back in the same copy, as a third value."""
    host = (buf[:3] if extra is None else torch.cat([buf[:3], extra.reshape(1)])).cpu()
    bits = int(host[2:3].view(torch.int32).item()) & 0xFFFFFFFF
    if bits & _lib.STATUS_DIFF_RANK and pt is not None:
        _raise_flagged_rank(x, pt)
    if bits:
        raise _lib.UwieError(f"device status 0x{bits:x}: the results of the calls since the last check are not valid "
                             "(include/uwie.h UWIE_STATUS_*)")
    if extra is not None:
        return float(host[0]), float(host[1]), float(host[3])
    return float(host[0]), float(host[1])


class ReferenceLoss(torch.nn.Module):
    """``deep_learning_parameters.ReferenceLoss`` (:170-196): ``loss, parts = crit(enhanced, reference)`` with
    ``loss = l1_weight * L1 + l2_weight * MSE`` (0-dim, with ``grad_fn``) and ``parts = {'l1': float, 'l2': float}``.

    float32 ROCm tensors of one shape take the device kernels (uwie_ref_loss_f32, one host read per call for ``parts``); the
    gradient of ``enhanced`` is torch CPU autograd's, bit for bit.  Other inputs -- different shapes (torch broadcasts them,
    with its warning), CPU tensors, other dtypes, a reference that requires grad -- go through torch's ``l1_loss`` /
    ``mse_loss``, as in the reference.

    ``crit.through(module, images, params, references)``: the same ``(loss, parts)`` for ``module(images, params)`` (a
    ``GatedDifferentiableEnhancement`` or ``DifferentiableEnhancement``) with the loss fused into the module's sweeps: no
    enhanced tensor is written, and the backward forms dL/d(enhanced) in registers.
    """

    def __init__(self, l1_weight=0.5, l2_weight=0.5, device: int | None = None):
        super().__init__()
        self.l1_weight = l1_weight
        self.l2_weight = l2_weight
        self.device = device

    @staticmethod
    def _takes(enhanced, reference) -> bool:
        return (isinstance(enhanced, torch.Tensor) and isinstance(reference, torch.Tensor) and enhanced.is_cuda
                and reference.is_cuda and enhanced.device == reference.device and enhanced.dtype == torch.float32
                and reference.dtype == torch.float32 and tuple(enhanced.shape) == tuple(reference.shape)
                and enhanced.numel() > 0 and enhanced.numel() % 3 == 0 and not reference.requires_grad)

    def forward(self, enhanced, reference):
        if not self._takes(enhanced, reference):
            l1 = torch.nn.functional.l1_loss(enhanced, reference)
            l2 = torch.nn.functional.mse_loss(enhanced, reference)
            return self.l1_weight * l1 + self.l2_weight * l2, {"l1": l1.item(), "l2": l2.item()}
        dev = get_device(enhanced.device.index)
        shape = tuple(enhanced.shape)
        if not (len(shape) == 4 and shape[1] == 3):
            shape = (1, 3, 1, enhanced.numel() // 3)  # the identity map sums every value: any layout
        sink = []
        l1, l2 = RefLossFunction.apply(enhanced.contiguous().view(shape), reference.contiguous().view(shape), dev, sink)
        host = sink[0][:2].cpu()
        return self.l1_weight * l1 + self.l2_weight * l2, {"l1": float(host[0]), "l2": float(host[1])}

    def through(self, module, images, params, references):
        """``crit(module(images, params), references)`` in one fused step: ``(loss, parts)``, one host read per call (the
        loss values and the device status together).  A gated module's unindexable sorted position raises the module's
        exception; a reference that is not float32 or not ``images``' shape raises ValueError."""
        if isinstance(references, torch.Tensor) and references.requires_grad:
            return self(module(images, params), references)
        sink = []
        dev, (l1, l2), x, pt = _module_loss(module, images, params, references, False, True, sink)
        v1, v2 = _read_loss(dev, sink[0], x, pt)
        return self.l1_weight * l1 + self.l2_weight * l2, {"l1": v1, "l2": v2}
