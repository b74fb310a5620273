"""Host-side mirror of the reference's enhancement API, driving the HIP kernels.

Reference surfaces mirrored here (same names, argument meaning and error behaviour):

* ``enhance(frame_u8)``                         -- the canonical ``enhance(img) -> img`` of SURVEY.md section 8:
  ``six_stadigy.py:406`` (u8 -> float32/255), ``:409-413`` (cast detection + correction),
  ``:427`` (``strategyN``), ``:430`` (``(y*255).astype(uint8)``);
* ``SixStrategies.strategy1_strong_dehazing`` ... ``strategy6_histogram_eq``, ``detect_image_type``,
  ``color_correction``                           -- ``six_stadigy.py:230-285,292-323``;
* ``EnhancementStrategies.apply_strategy(img, name, params)`` -- ``enhancement_strategies.py:477-508``.

Float images: a u8-derived image (``u8.astype(float32)/255`` possibly followed by ``color_correction``), which is what the
reference's pipelines pass (``six_stadigy.py:406``, ``main.py:108``), is recognised and takes the fast path that starts
from the u8 frame.  Any other float image in ``[0, 1]`` -- the reference's own harness inputs are ``np.random.rand``
(``enhancement_strategies.py:516``, ``example_usage.py:27,44,112``) -- takes the general float path
(``uwie_enhance_f32`` / ``uwie_enhance_f64``: same arithmetic, pixel values read from the float image, unfused):
float32 on both surfaces, float64 on the dict surface.  What is left raises ``UnsupportedInputError`` (float64 images on
the six_stadigy surface, whose functions are written for float32 frames; other dtypes) -- also from ``apply_strategy``,
whose swallow-and-return-the-input convention (ES:503-508) is for failures INSIDE a strategy: an input this build cannot
process is never reported as a successful pass-through.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
# the enhancement modules and ReferenceLoss live in modules.py; this module re-exports them
from .modules import (DifferentiableEnhancement, DiffEnhanceFunction, DiffEnhanceLossFunction,  # noqa: F401
                      GatedDifferentiableEnhancement, GatedDiffEnhanceFunction, GatedDiffEnhanceLossFunction, ReferenceLoss,
                      RefLossFunction, _image_batch, _loss_reference, _module_loss, _raise_rank_error, _read_loss)
from .runtime import Device, HandleOwner, get_device


class UnsupportedInputError(ValueError):
    """The float image is not u8-derived: this build has no device path for it (see the module docstring)."""


_F255 = np.float32(255.0)
_ATTEN = np.float32(0.85)


def _patch_needs_u8(frames, dark_patch):
    """dark_patch > 1 is built for u8 frames: a float image (which no u8 entry point takes anyway) is named as unsupported."""
    dtype = getattr(frames, "dtype", None)
    if int(dark_patch) > 1 and dtype is not None and dtype not in (np.uint8, torch.uint8):
        raise UnsupportedInputError(f"dark_patch > 1 takes uint8 frames or u8-derived float images, got {dtype}")


def _as_batch_u8(frames, dev: Device):
    """numpy/torch, [H,W,3] or [B,H,W,3] uint8 -> (cuda uint8 [B,H,W,3], was_numpy, was_single)."""
    was_numpy = isinstance(frames, np.ndarray)
    t = torch.from_numpy(np.ascontiguousarray(frames)) if was_numpy else frames
    if t.dtype != torch.uint8:
        raise TypeError(f"expected uint8 frames, got {t.dtype}")
    single = t.dim() == 3
    if single:
        t = t.unsqueeze(0)
    if t.dim() != 4 or t.shape[-1] != 3:
        raise ValueError(f"expected [H,W,3] or [B,H,W,3], got {tuple(t.shape)}")
    if t.numel() == 0:
        raise ValueError("empty image")
    return t.to(dev.torch_device).contiguous(), was_numpy, single


# include/uwie.h uwie_gray_world_u8: the columns of a row of its stats
GRAY_WORLD_STAT_NAMES = ("mean_r", "mean_g", "mean_b", "k_r", "k_b", "m_r", "m_g", "m_b", "gray", "s_r", "s_g", "s_b")
_GRAY_WORLD_KEYS = ("red", "blue", "max_gain")


def _gray_world_args(gray_world):
    """The ``gray_world=`` keyword of the enhance / select entry points -> None (no pre-pass) or the keyword arguments of
    ``gray_world()``: ``True`` means the defaults, a dict gives ``red`` / ``blue`` / ``max_gain``."""
    if gray_world is None or gray_world is False:
        return None
    if gray_world is True:
        return {}
    if isinstance(gray_world, dict):
        unknown = sorted(set(gray_world) - set(_GRAY_WORLD_KEYS))
        if unknown:
            raise KeyError(f"gray_world: unknown key(s) {unknown}; it takes {list(_GRAY_WORLD_KEYS)}")
        return {k: float(v) for k, v in gray_world.items()}
    raise TypeError(f"gray_world must be None, True or a dict of red / blue / max_gain, got {type(gray_world).__name__}")


def _gray_world_needs_u8(frames):
    dtype = getattr(frames, "dtype", None)
    if dtype is not None and dtype not in (np.uint8, torch.uint8):
        raise UnsupportedInputError(f"gray_world takes uint8 frames, got {dtype}")


def _as_balanced_batch_u8(frames, dev: Device, gray_world=None):
    """``_as_batch_u8`` with the gray-world pre-pass composed in front: ``f(x, gray_world=g) == f(gray_world(x, **g))`` bit for
    bit, for every caller.  ``gray_world=None`` is ``_as_batch_u8`` itself: no launch, no buffer."""
    g = _gray_world_args(gray_world)
    if g is not None:
        _gray_world_needs_u8(frames)
    batch, was_numpy, single = _as_batch_u8(frames, dev)
    if g is not None:
        batch, _ = dev.gray_world(batch, **g)  # a new tensor: the caller's frames stay as they are
    return batch, was_numpy, single


def _finish(t, was_numpy, single, dev: Device | None = None):
    if single:
        t = t[0]
    if not was_numpy:
        return t
    out = t.cpu().numpy()
    if dev is not None:
        dev.check_status()  # (the copy above synchronised already: this only reads the device's status word)
    return out


def gray_world(frames, red: float = 1.0, blue: float = 0.0, max_gain: float = 0.0, device: int | None = None,
               return_stats: bool = False):
    """Gray-world white balance with red-channel compensation (Ancuti et al. 2018 eq. 4-5, then Buchsbaum's gray world) in the
    fixed form include/uwie.h states (uwie_gray_world_u8; an extension without a reference counterpart), on the device: uint8
    ``[H,W,3]`` / ``[B,H,W,3]``, NumPy or a torch ROCm tensor -> the balanced frames, of the same kind.  ``red`` / ``blue``: how
    much of the green mean's lead the red / blue channel is given before the balance (the papers' alpha, 0 .. 1; 0 / 0 is plain
    gray-world); ``max_gain``: upper bound of the three channel gains (0: none, else >= 1).  Every frame of a batch has its own
    gains.  With ``return_stats`` the result is ``(out, stats)``, stats float64 ``(12,)`` / ``(B, 12)`` in
    ``GRAY_WORLD_STAT_NAMES`` order."""
    _gray_world_needs_u8(frames)
    dev = get_device(device)
    batch, was_numpy, single = _as_batch_u8(frames, dev)
    out, stats = dev.gray_world(batch, red=red, blue=blue, max_gain=max_gain, want_stats=return_stats)
    if not return_stats:
        return _finish(out, was_numpy, single, dev)
    return _finish(out, was_numpy, single, dev), _finish(stats, was_numpy, single)


def fusion_levels(H: int, W: int) -> int:
    """What ``fusion(levels=None)`` uses: min(6, max(1, floor(log2(min(H, W))) - 2)), a coarsest level of at least 4 points."""
    return min(6, max(1, int(min(H, W)).bit_length() - 3))


def fusion(frames, gamma: float = 2.2, levels: int | None = None, gray_world=True, return_parts: bool = False,
           device: int | None = None):
    """Ancuti et al. 2018's colour balance and multi-scale fusion in the fixed form include/uwie.h states (uwie_fusion_u8; an
    extension without a reference counterpart), on the device: uint8 ``[H,W,3]`` / ``[B,H,W,3]``, NumPy or a torch ROCm tensor
    -> the fused frames, of the same kind.  The frames are balanced by ``gray_world`` first (``True``, the default and the
    paper's pipeline, or a dict of ``red`` / ``blue`` / ``max_gain``; ``None`` fuses the frames as given):
    ``fusion(x, gray_world=g)`` is ``fusion(gray_world(x, **g), gray_world=None)``.  From the balanced frame a gamma-corrected
    input (``gamma``, 0 < gamma <= 8) and a sharpened one are blended over a Laplacian pyramid of ``levels`` levels (1 .. 8;
    ``None``: ``fusion_levels(H, W)``) with weights from Laplacian contrast, saliency and saturation.  With ``return_parts``
    the result is ``(out, (in1, in2, weight))``: the two inputs and the float64 normalised weight of the first."""
    _gray_world_needs_u8(frames)
    dev = get_device(device)
    batch, was_numpy, single = _as_balanced_batch_u8(frames, dev, gray_world)
    if levels is None:
        levels = fusion_levels(batch.shape[1], batch.shape[2])
    out, parts = dev.fusion(batch, gamma=gamma, levels=levels, want_parts=return_parts)
    if not return_parts:
        return _finish(out, was_numpy, single, dev)
    return _finish(out, was_numpy, single, dev), tuple(_finish(t, was_numpy, single, dev if t.dtype == torch.uint8 else None) for t in parts)


def enhance(frames, strategy: int = 2, cast_correct: bool = True, device: int | None = None, return_float: bool = False,
            gray_world=None, **overrides):
    """Canonical ``enhance(u8 RGB) -> u8 RGB`` (six_stadigy.py:406-431) for one frame or a batch.

    ``frames``: uint8 ``[H,W,3]`` / ``[B,H,W,3]``, NumPy (copied to HBM and back) or a torch ROCm tensor (stays on
    the device).  ``strategy`` selects ``strategy1..6`` (default 2, medium dehazing).  ``overrides`` set
    ``uwie_params`` fields (e.g. ``omega=0.6, gf_ksize=20``; ``dark_patch=15`` takes the dark channel over a 15 x 15 patch,
    an extension without a reference counterpart: include/uwie.h).  ``gray_world`` (``True`` or a dict of ``red`` / ``blue`` /
    ``max_gain``; default ``None``: nothing changes) balances the frames first: ``enhance(x, gray_world=g, ...)`` is
    ``enhance(gray_world(x, **g), ...)``, so cast detection sees the balanced frame.
    """
    dev = get_device(device)
    _patch_needs_u8(frames, overrides.get("dark_patch", 1))
    batch, was_numpy, single = _as_balanced_batch_u8(frames, dev, gray_world)
    p = dev.params(_lib.SURFACE_SIX, int(strategy), cast_correct=int(bool(cast_correct)), **overrides)
    out, outf = dev.enhance_u8(batch, p, want_float=return_float)
    return _finish(outf if return_float else out, was_numpy, single, dev)


# ------------------------------------------------------------------ the batch driver's fan-out (six_stadigy.py:330-520)
# (name, description) of the driver's strategy table, six_stadigy.py:344-351
DRIVER_STRATEGIES = (
    ("strong_dehazing", "強力去霧"), ("medium_dehazing", "中度去霧"), ("light_dehazing", "輕度去霧"),
    ("clahe_enhancement", "CLAHE增強"), ("white_balance", "白平衡主導"), ("histogram_eq", "直方圖均衡"),
)
CAST_NAMES = ("normal", "greenish", "bluish")


def enhance_all(frames, cast_correct: bool = True, device: int | None = None, dark_patch: int = 1, gray_world=None):
    """All six strategies of every frame in one call: one cast detection and one atmospheric-light quadtree per frame
    (strategies 1-3 share it), like the inner loop of ``process_all_images_all_strategies`` (six_stadigy.py:398-431).

    Returns ``(outputs, image_types)``: ``outputs[name]`` is the uint8 batch of that strategy (keys in the driver's
    order, see ``DRIVER_STRATEGIES``), ``image_types`` the list of ``"normal" / "greenish" / "bluish"`` per frame.
    ``dark_patch`` (default 1, the reference) applies to the dehazing strategies 1-3.  ``gray_world``: as for ``enhance``.
    """
    dev = get_device(device)
    batch, was_numpy, single = _as_balanced_batch_u8(frames, dev, gray_world)
    out, kind = dev.enhance_all_u8(batch, cast_correct, dark_patch=dark_patch)
    types = [CAST_NAMES[int(k)] for k in kind.cpu().tolist()]
    outs = {name: _finish(out[i], was_numpy, single, dev) for i, (name, _) in enumerate(DRIVER_STRATEGIES)}
    return outs, types


def process_batch(frames, filenames=None, device: int | None = None, compute=None, compute_one=None):
    """Host mirror of the driver's bookkeeping (six_stadigy.py:369-520) for frames that are already decoded: returns
    ``(outputs, log_rows, stats)`` where ``log_rows`` has one dict per (image, strategy) with the driver's columns
    (``filename, image_type, strategy, strategy_desc, status, output_path, processing_time``) and ``stats`` its counters.
    File I/O (glob / imread / imwrite / CSV) stays with the caller: ``output_path`` is empty for a success (the caller
    fills it in when it writes the file) and ``"Error: <first 50 characters>"`` for a failure, as in S6:464-478.

    The whole batch goes through ONE fused call (``enhance_all``: one cast detection and one quadtree per frame).  Failure
    handling follows the reference's two ``try`` levels (S6:395,424): if the fused call raises, every image is retried on
    its own; if an image's fused call raises, its six strategies run one by one, and a strategy that raises becomes a row
    with ``status='failed'``, ``processing_time='N/A'`` and counts in ``failed_outputs`` while the other five still succeed
    (S6:464-480); an image none of whose strategies succeeds counts in ``failed_images`` (S6:484-488), and one whose cast
    detection itself fails gets no rows at all (S6:508-510).  ``processing_time`` of a success is the time since the image
    started (S6:457): the image's share of the fused call, or the running time of the one-by-one fallback.
    ``outputs[name]`` is a list with one uint8 frame (or ``None`` for a failed output) per image.
    ``frames``: ``[B,H,W,3]`` uint8 or a list of ``[H,W,3]`` frames (frames of different sizes run image by image).
    ``compute`` / ``compute_one`` (tests) replace ``enhance_all(frames)`` / ``enhance(frame, strategy=k)``.
    """
    import time

    n = len(frames)
    filenames = list(filenames) if filenames is not None else [f"frame_{i:05d}" for i in range(n)]
    if len(filenames) != n:
        raise ValueError("one filename per frame")
    run_all = compute or (lambda f: enhance_all(f, device=device))
    run_one = compute_one or (lambda f, k: enhance(f, strategy=k, device=device))
    stats = {"total_images": n, "processed_images": 0, "failed_images": 0, "total_outputs": 0, "successful_outputs": 0,
             "failed_outputs": 0, "image_types": {"greenish": 0, "bluish": 0, "normal": 0}}
    names = [name for name, _ in DRIVER_STRATEGIES]
    outs = {name: [None] * n for name in names}
    # per image: (image_type, [(ok, time string or error message)] * 6) or None when the image failed before its strategy loop
    results = [None] * n

    def fused(idx, batch):
        t0 = time.time()
        o, types = run_all(batch)
        share = (time.time() - t0) / max(len(idx), 1)
        for j, i in enumerate(idx):
            for name in names:
                outs[name][i] = o[name][j]
            results[i] = (types[j], [(True, f"{share:.2f}s")] * len(names))

    def one_by_one(i):
        frame = frames[i]
        t0 = time.time()
        x = np.asarray(frame.cpu() if hasattr(frame, "cpu") else frame)
        try:
            # (the image_type column only; the strategies detect the cast again themselves, with the same result)
            kind = detect_image_type(x, device=device) if compute_one is None else "normal"
        except Exception:  # noqa: BLE001 - S6:508: the image fails as a whole
            return
        rows = []
        for k, name in enumerate(names, start=1):
            try:
                outs[name][i] = run_one(frame, k)
                rows.append((True, f"{time.time() - t0:.2f}s"))
            except Exception as e:  # noqa: BLE001 - S6:464: any failure of a strategy is a failed row
                outs[name][i] = None
                rows.append((False, str(e)[:50]))
        results[i] = (kind, rows)

    uniform = hasattr(frames, "shape") or len({tuple(np.shape(f)) for f in frames}) <= 1
    done = False
    if uniform and n > 0:
        try:
            batch = frames if hasattr(frames, "shape") else np.stack([np.asarray(f) for f in frames])
            fused(list(range(n)), batch)
            done = True
        except Exception:  # noqa: BLE001
            done = False
    if not done:
        for i in range(n):
            try:
                f = frames[i]
                fused([i], f[None] if hasattr(f, "shape") else np.asarray(f)[None])
            except Exception:  # noqa: BLE001
                one_by_one(i)

    rows = []
    for i, fname in enumerate(filenames):
        if results[i] is None:
            stats["failed_images"] += 1
            continue
        kind, per = results[i]
        stats["image_types"][kind] += 1
        good = 0
        for (sname, sdesc), (ok, info) in zip(DRIVER_STRATEGIES, per):
            if ok:
                rows.append({"filename": fname, "image_type": kind, "strategy": sname, "strategy_desc": sdesc,
                             "status": "success", "output_path": "", "processing_time": info})
                stats["successful_outputs"] += 1
                good += 1
            else:
                rows.append({"filename": fname, "image_type": kind, "strategy": sname, "strategy_desc": sdesc,
                             "status": "failed", "output_path": f"Error: {info}", "processing_time": "N/A"})
                stats["failed_outputs"] += 1
        stats["processed_images" if good else "failed_images"] += 1
        stats["total_outputs"] += len(DRIVER_STRATEGIES)
    return outs, rows, stats


# ------------------------------------------------------------------ PerceptualLoss / CombinedLoss (vgg_16_UIE.py:257-303, N10)
VGG16_CHECKPOINT = "vgg16-397923af.pth"  # torchvision's file name for vgg16(pretrained=True)
_VGG_CONVS = ((0, 3, 64), (2, 64, 64), (5, 64, 128), (7, 128, 128), (10, 128, 256), (12, 256, 256), (14, 256, 256))


def _vgg_tensors(weights):
    """The 14 float32 CPU tensors of vgg16().features[:16] (weight, bias of convs 0, 2, 5, 7, 10, 12, 14) from ``weights``: a
    state dict with keys ``N.weight`` / ``N.bias`` or ``features.N.weight`` / ..., a path to one (torch.load,
    weights_only=True), or None: torchvision's cached checkpoint under torch.hub.get_dir()/checkpoints (never downloaded)."""
    if weights is None:
        path = os.path.join(torch.hub.get_dir(), "checkpoints", VGG16_CHECKPOINT)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"no VGG16 weights at {path} (pass weights=, or place torchvision's {VGG16_CHECKPOINT} "
                                    "there; nothing is downloaded)")
        weights = path
    if isinstance(weights, (str, os.PathLike)):
        weights = torch.load(weights, map_location="cpu", weights_only=True)
    out = []
    for i, cin, cout in _VGG_CONVS:
        for name, shape in (("weight", (cout, cin, 3, 3)), ("bias", (cout,))):
            key = f"{i}.{name}"
            if key not in weights:
                key = f"features.{i}.{name}"
            if key not in weights:
                raise ValueError(f"VGG16 weights: missing key '{i}.{name}' (or 'features.{i}.{name}')")
            t = torch.as_tensor(weights[key])
            if tuple(t.shape) != shape:
                raise ValueError(f"VGG16 weights: '{key}' has shape {tuple(t.shape)}, expected {shape}")
            out.append(t.detach().to(device="cpu", dtype=torch.float32).contiguous())
    return out


def vgg16_features16(weights=None) -> torch.nn.Sequential:
    """torchvision's ``vgg16().features[:16]`` (conv1_1 ... relu3_3) in plain torch.nn, frozen, in eval mode, on the CPU:
    the module PerceptualLoss computes and falls back to.  ``weights`` as in PerceptualLoss."""
    nn = torch.nn
    tensors = _vgg_tensors(weights)
    layers = []
    for i, cin, cout in _VGG_CONVS:
        if i in (5, 10):
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2, padding=0, dilation=1, ceil_mode=False))
        layers += [nn.Conv2d(cin, cout, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
    seq = nn.Sequential(*layers)
    with torch.no_grad():
        for k, (i, _, _) in enumerate(_VGG_CONVS):
            seq[i].weight.copy_(tensors[2 * k])
            seq[i].bias.copy_(tensors[2 * k + 1])
    for p in seq.parameters():
        p.requires_grad = False
    return seq.eval()


class PerceptualFunction(torch.autograd.Function):
    """``loss = PerceptualFunction.apply(pred, target, crit, dev, precision, sink)``: mse_loss(F(pred), F(target)) on the
    device (uwie_perceptual_f32), 0-dim float32; ``pred`` gets the gradient, ``target`` none.  ``sink`` (a list or None)
    receives the device buffer {loss}.  The device status word is left as it is (the kernels set no bit)."""

    @staticmethod
    def forward(ctx, pred, target, crit, dev, precision, sink=None):
        h = crit._handle(dev, precision)
        buf, ws = dev.perceptual_f32(h, precision, pred, target)
        ctx.dev, ctx.crit, ctx.handle, ctx.ws, ctx.shape = dev, crit, h, ws, tuple(pred.shape)
        if sink is not None:
            sink.append(buf)
        return buf[0]

    @staticmethod
    def backward(ctx, grad):
        if grad is None or not ctx.needs_input_grad[0]:
            return (None,) * 6
        return (ctx.dev.perceptual_bwd_f32(ctx.handle, ctx.shape, ctx.ws, grad),) + (None,) * 5


class PerceptualLoss(HandleOwner, torch.nn.Module):
    """``vgg_16_UIE.PerceptualLoss`` (:257-269): ``crit(pred, target) = mse_loss(F(pred), F(target))`` with F =
    vgg16().features[:16], a 0-dim loss with ``grad_fn``.

    float32 ``(B, 3, H, W)`` ROCm tensors of one shape, with a ``target`` that does not require grad, take the device kernels
    (k_vgg.hip): the float32 route, or inside ``torch.autocast("cuda", dtype=torch.float16)`` autocast's float16 route.  Other
    inputs -- CPU tensors, other dtypes or shapes, a bfloat16 autocast region, a target that requires grad -- go through
    ``vgg16_features16`` in torch.  ``H`` or ``W`` below 4 raises RuntimeError (a max-pool output would be empty), as torch
    does.  ``weights``: a state dict (``N.weight`` or ``features.N.weight`` keys), a path, or None for torchvision's cached
    ``vgg16-397923af.pth`` (FileNotFoundError when it is absent; nothing is downloaded).

    The weights are a frozen copy, read once: they are not parameters or buffers of this module (``state_dict()``,
    ``.to()`` and ``load_state_dict`` do not see them; make a new PerceptualLoss for other weights).  The kernels take them
    packed per GPU and precision (uwie_vgg_create).  ``device`` (a GPU index) packs both precisions there at construction;
    otherwise each is packed on the inputs' GPU at its first use.  Packing and ``close()`` (also run by ``__del__``)
    synchronise that GPU: do not let either happen inside a CUDA graph capture.
    """

    def __init__(self, weights=None, device: int | None = None):
        super().__init__()
        self._tensors = _vgg_tensors(weights)
        self.device = device
        self._torch = {}
        if device is not None:
            dev = get_device(device)
            for precision in (_lib.VGG_F32, _lib.VGG_F16):
                self._handle(dev, precision)

    def _create_handle(self, dev: Device, precision: int):
        return dev.vgg_create(torch.cat([t.reshape(-1) for t in self._tensors]), precision)

    _destroy_handle = staticmethod(Device.vgg_destroy)

    def features(self, device=None) -> torch.nn.Sequential:
        """The torch module of these weights (vgg16_features16) on ``device`` (default: CPU), cached."""
        key = str(torch.device("cpu") if device is None else torch.device(device))
        if key not in self._torch:
            state = {f"{i}.{n}": self._tensors[2 * k + j] for k, (i, _, _) in enumerate(_VGG_CONVS) for j, n in enumerate(("weight", "bias"))}
            self._torch[key] = vgg16_features16(state).to(key)
        return self._torch[key]

    @staticmethod
    def _route(pred, target):
        """_lib.VGG_F32 / VGG_F16 for inputs the kernels take, None for the torch route."""
        if not (isinstance(pred, torch.Tensor) and isinstance(target, torch.Tensor) and pred.is_cuda and target.is_cuda
                and pred.device == target.device and pred.dtype == torch.float32 and target.dtype == torch.float32
                and pred.dim() == 4 and pred.shape[1] == 3 and tuple(pred.shape) == tuple(target.shape)
                and pred.shape[0] > 0 and not target.requires_grad):
            return None
        if torch.is_autocast_enabled("cuda"):
            return _lib.VGG_F16 if torch.get_autocast_dtype("cuda") == torch.float16 else None
        return _lib.VGG_F32

    @staticmethod
    def _check_size(x):
        H, W = int(x.shape[2]), int(x.shape[3])
        if H < 4 or W < 4:  # torch's max_pool2d message for the pool whose output is empty
            h, w, c = (H, W, 64) if H < 2 or W < 2 else (H // 2, W // 2, 128)
            raise RuntimeError(f"Given input size: ({c}x{h}x{w}). Calculated output size: ({c}x{h // 2}x{w // 2}). "
                               "Output size is too small")

    def _torch_loss(self, pred, target):
        vgg = self.features(pred.device if isinstance(pred, torch.Tensor) else None)
        return torch.nn.functional.mse_loss(vgg(pred), vgg(target))

    def _device_loss(self, pred, target, precision, sink=None):
        self._check_size(pred)
        dev = get_device(pred.device.index)
        return PerceptualFunction.apply(pred.contiguous(), target.contiguous(), self, dev, precision, sink)

    def forward(self, pred, target):
        precision = self._route(pred, target)
        if precision is None:
            return self._torch_loss(pred, target)
        return self._device_loss(pred, target, precision)


class CombinedLoss(torch.nn.Module):
    """``vgg_16_UIE.CombinedLoss`` (:272-303), ImprovedTrainer's criterion: ``total, parts = crit(enhanced, reference)`` with
    ``total = l1_weight * L1 + l2_weight * MSE + perceptual_weight * PerceptualLoss`` and ``parts = {'l1', 'l2',
    'perceptual'}`` as Python floats, all three from one host read on the device route (the reference makes three .item()
    calls).  L1 and MSE take ReferenceLoss's kernels, the perceptual term PerceptualLoss's; inputs those do not take go
    through torch as in the reference.

    ``crit.through(module, images, params, references)``: the same for ``module(images, params)`` (either enhancement
    module), with L1 / MSE fused into the module's sweeps (``module.with_loss``) and the perceptual gradient entering the
    module's fused backward as its ``grad_out``.
    """

    def __init__(self, l1_weight=0.3, l2_weight=0.5, perceptual_weight=0.2, weights=None, device: int | None = None):
        super().__init__()
        self.l1_weight = l1_weight
        self.l2_weight = l2_weight
        self.perceptual_weight = perceptual_weight
        self.perceptual_loss = PerceptualLoss(weights, device)

    def _total(self, l1, l2, p):
        return self.l1_weight * l1 + self.l2_weight * l2 + self.perceptual_weight * p

    def forward(self, enhanced, reference):
        precision = PerceptualLoss._route(enhanced, reference)
        if precision is None or not ReferenceLoss._takes(enhanced, reference):
            l1 = torch.nn.functional.l1_loss(enhanced, reference)
            l2 = torch.nn.functional.mse_loss(enhanced, reference)
            p = self.perceptual_loss(enhanced, reference)
            return self._total(l1, l2, p), {"l1": l1.item(), "l2": l2.item(), "perceptual": p.item()}
        PerceptualLoss._check_size(enhanced)
        dev = get_device(enhanced.device.index)
        sink = []
        enhanced, reference = enhanced.contiguous(), reference.contiguous()
        l1, l2 = RefLossFunction.apply(enhanced, reference, dev, sink)
        p = self.perceptual_loss._device_loss(enhanced, reference, precision, sink)
        host = torch.cat([sink[0][:2], sink[1][:1]]).cpu()
        return self._total(l1, l2, p), {"l1": float(host[0]), "l2": float(host[1]), "perceptual": float(host[2])}

    def through(self, module, images, params, references):
        """``crit(module(images, params), references)`` with L1 / MSE fused into the module's step: ``(total, parts)``, one
        host read per call (the three values and the device status together).  Errors as ``ReferenceLoss.through``."""
        if isinstance(references, torch.Tensor) and references.requires_grad:
            return self(module(images, params), references)
        sink = []
        dev, (out, l1, l2), x, pt = _module_loss(module, images, params, references, True, True, sink)
        ref = _loss_reference(dev, x, references)
        precision = PerceptualLoss._route(out, ref)
        if precision is None:
            p = self.perceptual_loss(out, ref)
            v1, v2 = _read_loss(dev, sink[0], x, pt)
            return self._total(l1, l2, p), {"l1": v1, "l2": v2, "perceptual": p.item()}
        psink = []
        p = self.perceptual_loss._device_loss(out, ref, precision, psink)
        v1, v2, vp = _read_loss(dev, sink[0], x, pt, psink[0][:1])
        return self._total(l1, l2, p), {"l1": v1, "l2": v2, "perceptual": vp}


# ------------------------------------------------------------------ ImprovedVGGParameterNet / EnhancementPredictor (N11)
PARAM_KEYS = ("omega", "gamma", "L_low", "L_high")  # param_heads order (vgg_16_UIE.py:186-191)
PARAM_RANGES = {"omega": (0.3, 0.9), "gamma": (1.0, 1.5), "L_low": (2.0, 15.0), "L_high": (60.0, 95.0)}  # :193-198
PREDICTOR_CLIP = {"omega": (0.1, 0.9), "gamma": (0.5, 3.0), "L_low": (1.0, 30.0), "L_high": (65.0, 99.0)}  # use_trained_model.py:74-77
_PN_CONVS = _VGG_CONVS + ((17, 256, 512), (19, 512, 512), (21, 512, 512))


def param_net_layout(use_features: bool = True, hidden_dim: int = 256):
    """``(key, shape)`` of every float tensor of ``ImprovedVGGParameterNet``'s state dict, in state-dict order without
    ``num_batches_tracked``: the order ``uwie_param_net_create`` takes them in (include/uwie.h)."""
    if hidden_dim != 256:
        raise ValueError(f"hidden_dim={hidden_dim}: the device network is built for hidden_dim=256 (use_trained_model.py:20)")
    h = hidden_dim
    out = []
    for i, cin, cout in _PN_CONVS:
        out += [(f"vgg_features.{i}.weight", (cout, cin, 3, 3)), (f"vgg_features.{i}.bias", (cout,))]

    def bn(prefix, c):
        return [(f"{prefix}.{n}", (c,)) for n in ("weight", "bias", "running_mean", "running_var")]

    out += [("feature_fusion.0.weight", (2 * h, 1024 + (79 if use_features else 0))), ("feature_fusion.0.bias", (2 * h,))]
    out += bn("feature_fusion.1", 2 * h)
    out += [("feature_fusion.4.weight", (h, 2 * h)), ("feature_fusion.4.bias", (h,))] + bn("feature_fusion.5", h)
    out += [("attention.0.weight", (h // 4, h)), ("attention.0.bias", (h // 4,)), ("attention.2.weight", (h, h // 4)),
            ("attention.2.bias", (h,))]
    for k in PARAM_KEYS:
        out += [(f"param_heads.{k}.0.weight", (h // 2, h)), (f"param_heads.{k}.0.bias", (h // 2,)),
                (f"param_heads.{k}.3.weight", (1, h // 2)), (f"param_heads.{k}.3.bias", (1,))]
    return out


def _param_net_state(weights, use_features: bool = True, hidden_dim: int = 256):
    """The validated float32 CPU tensors of ``param_net_layout`` from ``weights``: a state dict, a checkpoint dict holding
    one under ``'model_state_dict'`` (use_trained_model.py:23), or a path to either (torch.load, weights_only=True)."""
    layout = param_net_layout(use_features, hidden_dim)
    if isinstance(weights, (str, os.PathLike)):
        weights = torch.load(weights, map_location="cpu", weights_only=True)
    if "model_state_dict" in weights:
        weights = weights["model_state_dict"]
    out = {}
    for key, shape in layout:
        if key not in weights:
            raise ValueError(f"ImprovedVGGParameterNet weights: missing key '{key}'")
        t = torch.as_tensor(weights[key])
        if tuple(t.shape) != shape:
            raise ValueError(f"ImprovedVGGParameterNet weights: '{key}' has shape {tuple(t.shape)}, expected {shape}")
        out[key] = t.detach().to(device="cpu", dtype=torch.float32).contiguous()
    return out


class _ParamNetTorch(torch.nn.Module):
    """``vgg_16_UIE.ImprovedVGGParameterNet`` restated in plain torch.nn (no torchvision): the same modules under the same
    state-dict keys, the same forward."""

    def __init__(self, use_features: bool = True, hidden_dim: int = 256):
        super().__init__()
        nn = torch.nn
        self.use_features = use_features
        layers, cin = [], 3
        for v in (64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512):
            if v == "M":
                layers.append(nn.MaxPool2d(kernel_size=2, stride=2, padding=0, dilation=1, ceil_mode=False))
            else:
                layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
                cin = v
        self.vgg_features = nn.Sequential(*layers)  # vgg16().features[:23]
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.maxpool = nn.AdaptiveAvgPool2d((1, 1))  # sic (vgg_16_UIE.py:158)
        h = hidden_dim
        self.feature_fusion = nn.Sequential(nn.Linear(1024 + (79 if use_features else 0), 2 * h), nn.BatchNorm1d(2 * h),
                                            nn.ReLU(inplace=True), nn.Dropout(0.4), nn.Linear(2 * h, h), nn.BatchNorm1d(h),
                                            nn.ReLU(inplace=True), nn.Dropout(0.3))
        self.attention = nn.Sequential(nn.Linear(h, h // 4), nn.ReLU(inplace=True), nn.Linear(h // 4, h), nn.Sigmoid())
        self.param_heads = nn.ModuleDict({k: nn.Sequential(nn.Linear(h, h // 2), nn.ReLU(inplace=True), nn.Dropout(0.2),
                                                           nn.Linear(h // 2, 1)) for k in PARAM_KEYS})
        self.param_ranges = dict(PARAM_RANGES)

    def forward(self, img_tensor, feature_tensor=None, return_pooled: bool = False):
        B = img_tensor.size(0)
        vgg_feat = self.vgg_features(img_tensor)
        pooled = torch.cat([self.avgpool(vgg_feat).view(B, -1), self.maxpool(vgg_feat).view(B, -1)], dim=1)
        combined = pooled
        if self.use_features and feature_tensor is not None:
            if isinstance(feature_tensor, list):
                feature_tensor = torch.stack(feature_tensor)
            combined = torch.cat([pooled, feature_tensor.float().to(img_tensor.device)], dim=1)
        fused = self.feature_fusion(combined)
        fused = fused * self.attention(fused)
        params = {}
        for name, head in self.param_heads.items():
            lo, hi = self.param_ranges[name]
            params[name] = torch.sigmoid(head(fused)) * (hi - lo) + lo
        if return_pooled:
            params["pooled"] = pooled
        return params


def param_net_torch(weights, use_features: bool = True, hidden_dim: int = 256) -> torch.nn.Module:
    """``ImprovedVGGParameterNet`` with ``weights`` in plain torch.nn, frozen, in eval mode, on the CPU: the module
    ``VGGParameterNet`` falls back to.  ``weights`` as in VGGParameterNet."""
    state = _param_net_state(weights, use_features, hidden_dim)
    net = _ParamNetTorch(use_features, hidden_dim)
    missing, unexpected = net.load_state_dict(state, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing)
    for p in net.parameters():
        p.requires_grad = False
    return net.eval()


class VGGParameterNet(HandleOwner):
    """``vgg_16_UIE.ImprovedVGGParameterNet`` (:135-255) in eval mode on the device: ``net(img_tensor, feature_tensor)``
    returns the reference's dict of four ``(B, 1)`` float32 tensors (``omega``, ``gamma``, ``L_low``, ``L_high``);
    ``return_pooled=True`` adds ``'pooled'``, the ``[B, 1024]`` vector after the two global poolings.

    ``weights``: a state dict, a checkpoint dict with ``'model_state_dict'`` (use_trained_model.py:23), or a path to either
    (``torch.load(weights_only=True)``).  A missing key or a wrong shape is a ValueError naming the key; ``hidden_dim`` other
    than 256 is a ValueError.  float32 ``(B, 3, H, W)`` ROCm tensors outside an autocast region take the kernels (k_vgg.hip,
    k_param_net.hip); CPU tensors, other dtypes and autocast regions go through ``param_net_torch``.  ``H`` or ``W`` below
    8 raises RuntimeError (pool3's output would be empty), as torch does.  A ``use_features`` net called without features
    raises RuntimeError, as the reference's Linear does.  Inference only: the device route carries no gradient.

    The weights are a frozen copy, packed once per GPU (uwie_param_net_create; ``device`` packs at construction).  Packing
    and ``close()`` (also run by ``__del__``) synchronise that GPU."""

    def __init__(self, weights, use_features: bool = True, device: int | None = None, hidden_dim: int = 256):
        self.use_features = bool(use_features)
        self._state = _param_net_state(weights, self.use_features, hidden_dim)
        self.device = device
        self._torch = {}
        if device is not None:
            self._handle(get_device(device))

    def state_dict(self):
        return dict(self._state)

    def _create_handle(self, dev: Device):
        return dev.param_net_create(torch.cat([t.reshape(-1) for t in self._state.values()]), self.use_features)

    _destroy_handle = staticmethod(Device.param_net_destroy)

    def torch_module(self, device=None) -> torch.nn.Module:
        """The torch module of these weights (param_net_torch) on ``device`` (default: CPU), cached."""
        key = str(torch.device("cpu") if device is None else torch.device(device))
        if key not in self._torch:
            self._torch[key] = param_net_torch(self._state, self.use_features).to(key)
        return self._torch[key]

    @staticmethod
    def _takes(img) -> bool:
        return (isinstance(img, torch.Tensor) and img.is_cuda and img.dtype == torch.float32 and img.dim() == 4
                and img.shape[1] == 3 and img.shape[0] > 0 and not torch.is_autocast_enabled("cuda"))

    @staticmethod
    def _check_size(img):
        H, W = int(img.shape[2]), int(img.shape[3])
        if H < 8 or W < 8:  # torch's max_pool2d message for the pool whose output is empty
            c, h, w = ((64, H, W) if H < 2 or W < 2 else (128, H // 2, W // 2) if H < 4 or W < 4 else (256, H // 4, W // 4))
            raise RuntimeError(f"Given input size: ({c}x{h}x{w}). Calculated output size: ({c}x{h // 2}x{w // 2}). "
                               "Output size is too small")

    def _device_forward(self, dev: Device, img, features, want_pooled: bool = False):
        """(float32 [B,4], pooled or None) on ``dev`` for a float32 [B,3,H,W] ``img`` there and float32 [B,79] ``features``."""
        self._check_size(img)
        feats = None
        if self.use_features:
            if features is None:
                raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({img.shape[0]}x1024 and 1103x512): this "
                                   "network was built with use_features=True and needs the 79 features")
            if isinstance(features, list):
                features = torch.stack(features)
            feats = features.to(device=dev.torch_device, dtype=torch.float32)
            if tuple(feats.shape) != (img.shape[0], 79):
                raise RuntimeError(f"features: expected ({img.shape[0]}, 79), got {tuple(feats.shape)}")
        return dev.param_net_f32(self._handle(dev), img.contiguous(), feats, want_pooled)

    def forward(self, img_tensor, feature_tensor=None, return_pooled: bool = False):
        if not self._takes(img_tensor):
            dev = img_tensor.device if isinstance(img_tensor, torch.Tensor) else None
            return self.torch_module(dev)(img_tensor, feature_tensor, return_pooled=return_pooled)
        dev = get_device(img_tensor.device.index)
        out, pooled = self._device_forward(dev, img_tensor, feature_tensor, return_pooled)
        params = {k: out[:, i:i + 1] for i, k in enumerate(PARAM_KEYS)}
        if return_pooled:
            params["pooled"] = pooled
        return params

    __call__ = forward


class _FramePredictor:
    """What ``EnhancementPredictor`` and ``GatedEnhancementPredictor`` share: uint8 frames in, uint8 frames out.  A subclass
    has ``device``, ``_batch_u8(dev, u8) -> (out_u8, the module's float32 [B,4] parameters, the network's raw [B,4])`` with no
    host read between its stages, and ``_param_dicts(raw on the host)``: ``predict_parameters``' dict per row."""

    @staticmethod
    def _frame_u8(img):
        """The uint8 frame(s) behind ``img``: a uint8 array or tensor as it is, a float32 / float64 image equal to
        ``u8.astype(dtype) / 255`` as ``(img * 255).astype(uint8)`` (_preprocess_for_vgg's quantisation,
        use_trained_model.py:41)."""
        if isinstance(img, torch.Tensor) and img.dtype == torch.uint8:
            return img
        x = img.detach().cpu().numpy() if isinstance(img, torch.Tensor) else np.asarray(img)
        if x.dtype == np.uint8:
            return x
        if x.dtype not in (np.float32, np.float64):
            if x.dtype.kind == "f":
                raise UnsupportedInputError(f"EnhancementPredictor takes float32 or float64 images, got {x.dtype}")
            raise TypeError(f"expected uint8 frames or float images u8 / 255, got {x.dtype}")
        k = x.dtype.type(255)
        with np.errstate(invalid="ignore"):
            u8 = (x * k).astype(np.uint8)
        if not np.array_equal(u8.astype(x.dtype) / k, x):
            raise UnsupportedInputError("EnhancementPredictor takes uint8 frames or float images that are exactly u8 / 255")
        return u8

    @classmethod
    def _frames(cls, img, dev: Device):
        """(uint8 [B,H,W,3] on ``dev``, single) from a frame or a batch, uint8 or exactly u8 / 255."""
        batch, _, single = _as_batch_u8(cls._frame_u8(img), dev)
        return batch, single

    def enhance_batch_u8(self, frames):
        """``process_single_image``'s u8 result (use_trained_model.py:118-127) for a batch, as one device pipeline:
        ``(out_u8 [B,H,W,3] uint8 on the device, params float32 [B,4])``, ``params`` in the order and with the clamping that
        the class's enhancement module takes them.  ``frames`` as for ``enhance_batch``; ``out_u8`` equals
        ``(enhance_batch(frames) * 255).to(uint8)``.  The enhancement runs on the frames' bytes (DESIGN.md sections 16, 17): no
        float image is made.  No host read: ``Device.check_status`` reports an unindexable sorted position."""
        dev = get_device(self.device)
        u8, _ = self._frames(frames, dev)
        out, params, _ = self._batch_u8(dev, u8)
        return out, params

    def process_frames(self, frames, filenames=None):
        """``process_folder``'s loop (use_trained_model.py:145-164) without the file I/O, for decoded frames whose sizes may
        differ: ``frames`` is a sequence of HxWx3 frames (uint8, or float images equal to u8 / 255), ``filenames`` optional
        names for the messages.  Frames of equal shape go through one ``enhance_batch_u8`` pipeline per shape.  Returns
        ``(outputs, params)`` in input order: ``outputs[i]`` the enhanced uint8 HxWx3 NumPy frame, ``params[i]`` the dict
        ``predict_parameters`` gives for it.  A frame that raises does not stop the others (:163-164): its output is ``None``
        and its ``params`` entry is the exception's message (prefixed with its file name when names are given).  Input
        errors are found per frame before any launch; an error of a group's device run fails that group's frames."""
        frames = list(frames)
        if filenames is not None and len(filenames) != len(frames):
            raise ValueError(f"{len(filenames)} file names for {len(frames)} frames")
        dev = get_device(self.device)
        outputs, params = [None] * len(frames), [None] * len(frames)

        def fail(i, e):
            outputs[i] = None
            params[i] = f"{filenames[i]}: {e}" if filenames is not None else str(e)

        groups = {}
        for i, f in enumerate(frames):
            try:
                u8, single = self._frames(f, dev)
                if not single:
                    raise ValueError(f"process_frames takes HxWx3 frames, got {tuple(u8.shape)}")
                groups.setdefault(tuple(u8.shape), []).append((i, u8))
            except Exception as e:  # noqa: BLE001 - the reference's loop catches everything (:163)
                fail(i, e)

        for members in groups.values():
            try:
                out, _, raw = self._batch_u8(dev, torch.cat([u8 for _, u8 in members]))
                out, raw = out.cpu().numpy(), raw.cpu().numpy()
                dev.check_status()
            except Exception as e:  # noqa: BLE001 - a device error: the whole group fails, nothing is launched again for it
                for i, _ in members:
                    fail(i, e)
                continue
            for (i, _), o, d in zip(members, out, self._param_dicts(raw)):
                outputs[i], params[i] = o, d
        return outputs, params


class EnhancementPredictor(_FramePredictor):
    """``use_trained_model.EnhancementPredictor`` (:13-111) on the device, without torchvision or cv2: the network is
    ``VGGParameterNet`` (use_features=True), the VGG input ``vgg_input``, the features ``extract_all_features``, the
    enhancement ``DifferentiableEnhancement``.

    Images are uint8 RGB frames, or float32 / float64 images equal to ``u8.astype(dtype) / 255`` in their own dtype (what
    ``process_single_image`` makes, and NumPy's ``frame / 255``); any other float image raises ``UnsupportedInputError``.
    For such an image every step of the reference sees the frame's own values: ``(img * 255).astype(uint8)`` gives the
    frame back, and its float32 cast is ``u8.astype(float32) / 255`` for both dtypes.  ``predict_parameters(img)`` returns the reference's dict of six
    Python floats (clamped as :70-79); for a ``[B,H,W,3]`` batch, one float64 array per key.  ``enhance_image(img, params)``
    returns float32 HxWx3, clipped to [0, 1] with NaN and infinities replaced as :101-111.  ``enhance_batch(frames)`` runs
    the whole chain for a batch as one device pipeline (no host read between the stages) and returns ``[B,H,W,3]`` float32
    on the device, equal to B ``enhance_image`` calls bit for bit.  ``enhance_batch_u8(frames)`` goes on to the uint8
    frame ``process_single_image`` writes, in the byte domain; ``process_frames(list)`` is ``process_folder``'s loop for
    decoded frames of mixed sizes."""

    def __init__(self, weights, input_size: int = 224, device: int | None = None):
        self.input_size = int(input_size)
        self.device = device
        self.model = VGGParameterNet(weights, use_features=True, device=device)
        self.enhancer = DifferentiableEnhancement()
        self.enhancer.device = device

    def _raw(self, dev: Device, u8):
        """The network's float32 [B,4] (omega, gamma, L_low, L_high) for uint8 frames on the device."""
        _, _, x = dev.resize_rgb(u8, self.input_size, self.input_size, want_u8=False, want_f32=False,
                                 norm=(IMAGENET_MEAN, IMAGENET_STD))
        feats = dev.extract_features_u8(u8)
        return self.model._device_forward(dev, x, feats)[0]

    @staticmethod
    def _clip(dev: Device, raw):
        """float32(np.clip(float(v), lo, hi)) of the network's float32 [B,4] on the device: the reference's float64 clip
        (:74-77), then the float32 tensor of enhance_image (:96-103).  NaN stays NaN."""
        lo = torch.tensor([PREDICTOR_CLIP[k][0] for k in PARAM_KEYS], dtype=torch.float64, device=dev.torch_device)
        hi = torch.tensor([PREDICTOR_CLIP[k][1] for k in PARAM_KEYS], dtype=torch.float64, device=dev.torch_device)
        return torch.minimum(torch.maximum(raw.double(), lo), hi).float()

    def _clamped(self, dev: Device, u8):
        """float32 [B,4] (omega, gamma, L_low, L_high) on the device: the network's outputs, clipped (_clip)."""
        return self._clip(dev, self._raw(dev, u8))

    @staticmethod
    def _enhance(dev: Device, u8, cols):
        """DifferentiableEnhancement of u8 / 255 ([B,H,W,3] float32) with float32 [B,4] = L_low, L_high, omega, gamma."""
        return dev.diff_enhance_f32(dev.u8_to_f32(u8), cols, planar=False)

    def predict_parameters(self, img):
        dev = get_device(self.device)
        u8, single = self._frames(img, dev)
        raw = self._raw(dev, u8).double().cpu().numpy()
        dev.check_status()
        params = {}
        for i, k in enumerate(PARAM_KEYS):
            lo, hi = PREDICTOR_CLIP[k]
            params[k] = np.clip(raw[:, i], lo, hi)  # float(np.clip(float(v), lo, hi)), elementwise
        params["guided_radius"] = np.full(raw.shape[0], 15.0)
        params["use_gamma"] = np.full(raw.shape[0], 1.0)
        return {k: float(v[0]) for k, v in params.items()} if single else params

    def enhance_image(self, img, params=None):
        dev = get_device(self.device)
        u8, single = self._frames(img, dev)
        if not single:
            raise ValueError(f"enhance_image takes one HxWx3 image, got {tuple(u8.shape)} (enhance_batch takes batches)")
        if params is None:
            params = self.predict_parameters(img)
        cols = dev.tensor(np.array([[params["L_low"], params["L_high"], params["omega"], params["gamma"]]], np.float32))
        out = np.clip(self._enhance(dev, u8, cols)[0].cpu().numpy(), 0.0, 1.0)
        if not np.isfinite(out).all():
            out = np.clip(np.nan_to_num(out, nan=0.0, posinf=1.0, neginf=0.0), 0.0, 1.0)
        return out

    def enhance_batch(self, frames):
        dev = get_device(self.device)
        u8, _ = self._frames(frames, dev)
        clipped = self._clamped(dev, u8)
        out = self._enhance(dev, u8, clipped[:, [2, 3, 0, 1]].contiguous()).clamp_(0.0, 1.0)
        return torch.nan_to_num_(out, nan=0.0, posinf=1.0, neginf=0.0).clamp_(0.0, 1.0)

    def _batch_u8(self, dev: Device, u8):
        """(out_u8, clamped float32 [B,4], the network's raw float32 [B,4]) for uint8 frames on the device: the network, the
        clip and the module in the byte domain (uwie_diff_enhance_u8), no host read in between."""
        raw = self._raw(dev, u8)
        clipped = self._clip(dev, raw)
        out, _ = dev.diff_enhance_u8(u8, clipped[:, [2, 3, 0, 1]].contiguous(), 3, want_u8=True, want_f32=False)
        return out, clipped, raw

    @staticmethod
    def _param_dicts(raw):
        """predict_parameters' dicts (six Python floats each) from the network's raw outputs, float32 [B,4] on the host."""
        raw = np.asarray(raw, dtype=np.float64)
        dicts = []
        for row in raw:
            d = {k: float(np.clip(row[i], *PREDICTOR_CLIP[k])) for i, k in enumerate(PARAM_KEYS)}
            d["guided_radius"] = 15.0
            d["use_gamma"] = 1.0
            dicts.append(d)
        return dicts


# ------------------------------------------------------------------ ParameterPredictor / GatedEnhancementPredictor (N13)
GATED_PARAM_KEYS = ("gamma", "L_low", "L_high", "use_gamma")  # param_heads order (deep_learning_parameters.py:142-147)


def _gated_columns_dict(cols, keys=GATED_PARAM_KEYS):
    """``{key: its [B,1] column}`` for ``keys`` from a ``[B,4]`` tensor or array whose columns are in the gated module's order
    (``GatedDifferentiableEnhancement.KEYS``)."""
    at = {k: i for i, k in enumerate(GatedDifferentiableEnhancement.KEYS)}
    return {k: cols[:, at[k]:at[k] + 1] for k in keys}


def _feature_rows(dev: Device, rows, feature_dim: int, hidden_dim: int, promote_1d: bool = False):
    """Feature rows for the MLP on ``dev``: float32 or float64 ``[B, feature_dim]`` (NumPy or torch), B >= 1."""
    if not isinstance(rows, torch.Tensor):
        rows = torch.from_numpy(np.ascontiguousarray(rows))
    if rows.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"expected float32 or float64 feature rows, got {rows.dtype}")
    if promote_1d and rows.dim() == 1:
        rows = rows[None]
    if rows.dim() != 2 or rows.shape[1] != feature_dim or rows.shape[0] == 0:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({'x'.join(str(v) for v in rows.shape)} and "
                           f"{feature_dim}x{hidden_dim})")
    return rows.detach().to(dev.torch_device).contiguous()


def _predictor_state(state):
    """(validated float32 CPU tensors in state_dict() order, feature_dim, hidden_dim, num_blocks) of a
    ``deep_learning_parameters.ParameterPredictor``: ``state`` is its state dict, the module itself, a checkpoint dict with
    the ``'param_predictor'`` key (``EndToEndTrainer.save_model``) or a path to either.  The sizes come from the tensors'
    shapes; a missing key or a shape that does not fit raises ValueError naming the key."""
    if isinstance(state, (str, os.PathLike)):
        state = torch.load(state, map_location="cpu", weights_only=True)
    if isinstance(state, torch.nn.Module):
        state = state.state_dict()
    if "param_predictor" in state:
        state = state["param_predictor"]
    name = "ParameterPredictor state"
    first = "input_proj.0.weight"
    if first not in state:
        raise ValueError(f"{name}: missing key '{first}'")
    w = torch.as_tensor(state[first])
    if w.dim() != 2:
        raise ValueError(f"{name}: '{first}' has shape {tuple(w.shape)}, expected (hidden_dim, feature_dim)")
    h, f = int(w.shape[0]), int(w.shape[1])
    if h % 2 or not (2 <= h <= 1152 and 1 <= f <= 1152):
        raise ValueError(f"{name}: '{first}' has shape {tuple(w.shape)}: hidden_dim must be even and, like feature_dim, "
                         "at most 1152")
    nb = 0
    while f"res_blocks.{nb}.block.0.weight" in state:
        nb += 1
    layout = [(first, (h, f)), ("input_proj.0.bias", (h,))]
    for i in range(nb):
        layout += [(f"res_blocks.{i}.block.0.weight", (h, h)), (f"res_blocks.{i}.block.0.bias", (h,)),
                   (f"res_blocks.{i}.block.3.weight", (h, h)), (f"res_blocks.{i}.block.3.bias", (h,))]
    layout += [("output_proj.0.weight", (h // 2, h)), ("output_proj.0.bias", (h // 2,))]
    for k in GATED_PARAM_KEYS:
        layout += [(f"param_heads.{k}.weight", (1, h // 2)), (f"param_heads.{k}.bias", (1,))]
    out = {}
    for key, shape in layout:
        if key not in state:
            raise ValueError(f"{name}: missing key '{key}'")
        t = torch.as_tensor(state[key])
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: '{key}' has shape {tuple(t.shape)}, expected {shape}")
        out[key] = t.detach().to(device="cpu", dtype=torch.float32).contiguous()
    return out, f, h, nb


class ParameterPredictor(HandleOwner):
    """``deep_learning_parameters.ParameterPredictor`` (:114-163) in eval mode on the device (k_param_net.hip, DESIGN.md
    section 17).  ``state``: a state dict, the ``nn.Module``, or a checkpoint dict / path with the ``'param_predictor'`` key
    that ``EndToEndTrainer.save_model`` writes; ``feature_dim``, ``hidden_dim`` and ``num_blocks`` come from the tensors'
    shapes (ValueError naming the key when they do not fit).  ``predictor(rows)``: ``rows`` ``[B, feature_dim]`` float32 or
    float64 (NumPy or torch; float64 is rounded to float32, as ``torch.from_numpy(features).float()``), returns the
    reference's dict of four ``(B, 1)`` float32 tensors on the device (``gamma``, ``L_low``, ``L_high``, ``use_gamma``).
    Inference only.  The weights are a frozen copy, packed once per GPU; ``close()`` frees them."""

    def __init__(self, state, device: int | None = None):
        self._state, self.feature_dim, self.hidden_dim, self.num_blocks = _predictor_state(state)
        self.device = device
        if device is not None:
            self._handle(get_device(device))

    def state_dict(self):
        return dict(self._state)

    def _create_handle(self, dev: Device):
        flat = torch.cat([t.reshape(-1) for t in self._state.values()])
        return dev.mlp_create(flat, self.feature_dim, self.hidden_dim, self.num_blocks)

    _destroy_handle = staticmethod(Device.mlp_destroy)

    def columns(self, rows, dev: Device | None = None):
        """float32 ``[B,4]`` on the device in the gated module's order (``GatedDifferentiableEnhancement.KEYS``)."""
        dev = dev or get_device(self.device)
        rows = _feature_rows(dev, rows, self.feature_dim, self.hidden_dim, promote_1d=True)
        return dev.mlp_forward(self._handle(dev), rows, self.hidden_dim)

    def forward(self, rows):
        return _gated_columns_dict(self.columns(rows))

    __call__ = forward


class GatedEnhancementPredictor(_FramePredictor):
    """The inference route of ``EndToEndTrainer``'s stack (deep_learning_parameters.py) on the device, the counterpart of
    ``EnhancementPredictor``: ``FeatureExtractor`` rows -> ``ParameterPredictor`` -> the gated ``DifferentiableEnhancement``.
    ``state`` as for ``ParameterPredictor`` (``feature_dim`` 79).  Frames are uint8 RGB, or float images equal to
    ``u8 / 255`` (as ``EnhancementPredictor``); H and W even or 1 (an odd side has no DCT block: 74 features).

    ``predict_parameters(frames)``: the network's dict of Python floats for one frame, of float64 arrays for a batch.
    ``enhance_batch_u8(frames)``: ``(out_u8, params float32 [B,4] = L_low, L_high, use_gamma, gamma)`` on the device:
    features, MLP and the byte-domain module (uwie_diff_gated_u8) with no host read between the stages.
    ``enhance_batch(frames)``: the float32 route, ``u8_to_f32`` then ``GatedDifferentiableEnhancement.forward``, ``[B,H,W,3]``.
    ``process_frames`` as ``EnhancementPredictor.process_frames``.  ``validate_batch`` is ``EndToEndTrainer.validate``'s
    loop body."""

    def __init__(self, state, device: int | None = None):
        self.device = device
        self.model = ParameterPredictor(state, device=device)
        if self.model.feature_dim != 79:
            raise ValueError(f"ParameterPredictor state: 'input_proj.0.weight' takes {self.model.feature_dim} features, "
                             "FeatureExtractor gives 79")
        self.enhancer = GatedDifferentiableEnhancement()
        self.enhancer.device = device
        self.criterion = ReferenceLoss(0.5, 0.5, device=device)

    def _cols(self, dev: Device, u8):
        """The network's float32 [B,4] (gated order) for uint8 frames on the device."""
        rows = dev.feature_extractor(u8)
        if rows.shape[1] != 79:
            raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({rows.shape[0]}x{rows.shape[1]} and "
                               f"79x{self.model.hidden_dim}): a frame with an odd side has no DCT features")
        return self.model.columns(rows, dev)

    @staticmethod
    def _dict(cols):
        return {k: cols[:, i:i + 1] for i, k in enumerate(GatedDifferentiableEnhancement.KEYS)}

    def predict_parameters(self, frames):
        dev = get_device(self.device)
        u8, single = self._frames(frames, dev)
        raw = self._cols(dev, u8).double().cpu().numpy()
        dev.check_status()
        params = {k: v[:, 0] for k, v in _gated_columns_dict(raw).items()}
        return {k: float(v[0]) for k, v in params.items()} if single else params

    def enhance_batch(self, frames):
        dev = get_device(self.device)
        u8, _ = self._frames(frames, dev)
        cols = self._cols(dev, u8)
        with torch.no_grad():
            out = self.enhancer(dev.u8_to_f32(u8).permute(0, 3, 1, 2).contiguous(), self._dict(cols))
        return out.permute(0, 2, 3, 1).contiguous()

    def _batch_u8(self, dev: Device, u8):
        cols = self._cols(dev, u8)
        out, _ = dev.diff_gated_u8(u8, cols, want_u8=True, want_f32=False)
        return out, cols, cols

    @staticmethod
    def _param_dicts(raw):
        cols = _gated_columns_dict(np.asarray(raw, dtype=np.float64))
        return [{k: float(v[r, 0]) for k, v in cols.items()} for r in range(len(raw))]

    def validate_batch(self, images, references, features=None):
        """``EndToEndTrainer.validate``'s loop body (:316-329) for one batch: ``images`` / ``references`` float32
        ``(B,3,H,W)``, ``features`` ``(B,79)`` (None: ``FeatureExtractor``'s rows of the images).  Returns
        ``(loss, {'l1', 'l2'})`` from ``ReferenceLoss(0.5, 0.5).through(GatedDifferentiableEnhancement(), ...)`` under
        ``no_grad``, with one host read."""
        dev = get_device(self.device)
        x = images.to(dev.torch_device) if isinstance(images, torch.Tensor) else dev.tensor(np.asarray(images))
        with torch.no_grad():
            if features is None:
                nhwc = x.permute(0, 2, 3, 1).contiguous()
                features = dev.feature_extractor((nhwc * 255).to(torch.uint8), nhwc)
            cols = self.model.columns(features, dev)
            return self.criterion.through(self.enhancer, x, self._dict(cols), references)


# ------------------------------------------------------------------ EndToEndTrainer (N14)
class _TrainerPredictor:
    """``EndToEndTrainer.param_predictor``: the trainer's current weights behind ``ParameterPredictor``'s eval forward."""

    def __init__(self, trainer):
        self._trainer = trainer
        self.feature_dim, self.hidden_dim, self.num_blocks = trainer.feature_dim, trainer.hidden_dim, trainer.num_blocks
        self.device = trainer.device

    def state_dict(self):
        return self._trainer.state_dict()

    def columns(self, rows, dev: Device | None = None):
        dev = dev or get_device(self.device)
        return dev.mlp_trainer_eval(self._trainer._handle, self._trainer._rows(dev, rows), self.hidden_dim)

    forward = __call__ = ParameterPredictor.forward


class EndToEndTrainer(HandleOwner):
    """``deep_learning_parameters.EndToEndTrainer`` (:253-349) on the device (k_mlp_train.hip).
    ``state_or_predictor``: a ``uw.ParameterPredictor`` or anything it takes (a state dict, the module, a checkpoint or its
    path).  The trainer owns the weights, their gradients and Adam's moments on the GPU; the reference's hyperparameters are
    the defaults (Adam lr 1e-4, betas (0.9, 0.999), eps 1e-8; ``clip_grad_norm_`` at 1.0; every Dropout at 0.3).

    ``train_step(images, references, features=None, masks=None)``: ``train_epoch``'s loop body (:273-298): features
    (``None``: ``FeatureExtractor``'s rows of the images) -> train-mode MLP -> gated enhancement and ``ReferenceLoss`` in one
    sweep -> their backward -> the MLP's backward -> clip and Adam.  Returns ``(loss, {'l1', 'l2'})`` as Python floats; the
    loss is the one host read.  ``masks``: uint8 ``[1 + 2 * num_blocks, B, hidden]`` keep bits in the Dropouts' call order
    (``None``: drawn from ``(seed, step)``).
    ``train_epoch(batches)`` / ``validate(batches)``: the reference's dict batches (``'image'``, ``'reference'``,
    ``'features'``) -> ``(avg_loss, {'l1', 'l2'})``.  ``param_predictor``: the current weights as an eval forward.
    ``save_model`` / ``load_model``: the reference's checkpoint, ``torch.optim.Adam``'s state dict included."""

    BETAS, EPS = (0.9, 0.999), 1e-8

    def __init__(self, state_or_predictor, device: int | None = None, lr: float = 1e-4, max_norm: float = 1.0, dropout: float = 0.3,
                 seed: int = 0):
        if hasattr(state_or_predictor, "state_dict") and not isinstance(state_or_predictor, torch.nn.Module):
            state_or_predictor = state_or_predictor.state_dict()
        state, self.feature_dim, self.hidden_dim, self.num_blocks = _predictor_state(state_or_predictor)
        self._layout = [(k, tuple(v.shape)) for k, v in state.items()]
        self._count = sum(int(v.numel()) for v in state.values())
        self.device, self.lr, self.betas, self.eps = device, float(lr), self.BETAS, self.EPS
        self.max_norm, self.dropout, self.seed = float(max_norm), float(dropout), int(seed)
        dev = get_device(device)
        self._index = dev.index
        flat = torch.cat([t.reshape(-1) for t in state.values()])
        self._handles = {(dev.index,): (dev, dev.mlp_trainer_create(flat, self.feature_dim, self.hidden_dim, self.num_blocks))}
        self.param_predictor = _TrainerPredictor(self)
        self.enhancement = GatedDifferentiableEnhancement()
        self.enhancement.device = device
        self.criterion = ReferenceLoss(0.5, 0.5, device=device)
        self._grad_loss = dev.tensor(np.array([0.5, 0.5], dtype=np.float32))  # d loss / d l1, d loss / d l2 (:190)

    _destroy_handle = staticmethod(Device.mlp_trainer_destroy)

    @property
    def _handle(self):
        """the one uwie_mlp_trainer, made by ``__init__`` from the initial state; None after ``close()``"""
        return next(iter(self._handles.values()), (None, None))[1]

    @property
    def step_count(self) -> int:
        return int(get_device(self._index).lib.uwie_mlp_trainer_step_count(self._handle))

    # ---- state
    def _free_of_gradient(self):
        """indices (in ``state_dict()`` order) of the L_low / L_high heads' tensors: no gradient in the reference, so no
        Adam state"""
        return {i for i, (k, _) in enumerate(self._layout) if k.startswith(("param_heads.L_low.", "param_heads.L_high."))}

    def _split(self, flat):
        out, at = {}, 0
        flat = flat.cpu()
        for key, shape in self._layout:
            n = int(np.prod(shape))
            out[key] = flat[at:at + n].reshape(shape).clone()
            at += n
        return out

    def _array(self, which: int):
        return self._split(get_device(self._index).mlp_trainer_get(self._handle, which, self._count))

    def state_dict(self):
        return self._array(_lib.TRAINER_PARAMS)

    def gradients(self):
        """the gradients of the last ``train_step`` (clipped, as ``p.grad`` after ``clip_grad_norm_``), by key"""
        return self._array(_lib.TRAINER_GRADS)

    def _set(self, which: int, tensors):
        flat = torch.cat([torch.as_tensor(tensors[k]).detach().to(dtype=torch.float32, device="cpu").reshape(-1) for k, _ in self._layout])
        get_device(self._index).mlp_trainer_set(self._handle, which, flat)

    def optimizer_state_dict(self):
        """``torch.optim.Adam(...).state_dict()`` of this trainer: no ``state`` entry for the gradient-free heads, ``step`` a
        float32 0-dim tensor; empty ``state`` before the first step."""
        n = len(self._layout)
        probe = torch.optim.Adam([torch.nn.Parameter(torch.zeros(())) for _ in range(n)], lr=self.lr, betas=self.betas, eps=self.eps)
        sd = probe.state_dict()
        step = self.step_count
        if step > 0:
            m, v, skip = self._array(_lib.TRAINER_EXP_AVG), self._array(_lib.TRAINER_EXP_AVG_SQ), self._free_of_gradient()
            sd["state"] = {i: {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": m[k], "exp_avg_sq": v[k]}
                           for i, (k, _) in enumerate(self._layout) if i not in skip}
        return sd

    def save_model(self, path):
        torch.save({"param_predictor": self.state_dict(), "optimizer": self.optimizer_state_dict()}, path)

    def load_model(self, path):
        ckpt = path if isinstance(path, dict) else torch.load(path, map_location="cpu", weights_only=False)
        state, f, h, nb = _predictor_state(ckpt["param_predictor"])
        if (f, h, nb) != (self.feature_dim, self.hidden_dim, self.num_blocks):
            raise ValueError(f"checkpoint of a ({f}, {h}, {nb}) network, this trainer holds ({self.feature_dim}, {self.hidden_dim}, "
                             f"{self.num_blocks})")
        opt = ckpt["optimizer"]
        entries, steps = opt.get("state", {}), set()
        zeros = {k: torch.zeros(shape) for k, shape in self._layout}
        m, v = dict(zeros), dict(zeros)
        for i, (k, shape) in enumerate(self._layout):
            e = entries.get(i)
            if e is None:
                continue
            if tuple(e["exp_avg"].shape) != shape or tuple(e["exp_avg_sq"].shape) != shape:
                raise ValueError(f"optimizer state {i} does not have the shape of '{k}' {shape}")
            m[k], v[k] = e["exp_avg"], e["exp_avg_sq"]
            steps.add(int(float(e["step"])))
        if len(steps) > 1:
            raise ValueError(f"optimizer state with different step counts {sorted(steps)}")
        dev = get_device(self._index)
        self._set(_lib.TRAINER_PARAMS, state)
        self._set(_lib.TRAINER_EXP_AVG, m)
        self._set(_lib.TRAINER_EXP_AVG_SQ, v)
        _lib.check(dev.lib.uwie_mlp_trainer_set_step_count(self._handle, steps.pop() if steps else 0))
        for g in opt.get("param_groups", [])[:1]:
            self.lr, self.betas, self.eps = float(g["lr"]), tuple(float(b) for b in g["betas"]), float(g["eps"])

    # ---- the step
    def _rows(self, dev: Device, rows):
        return _feature_rows(dev, rows, self.feature_dim, self.hidden_dim)

    def _features(self, dev: Device, x, features):
        if features is None:
            nhwc = x.permute(0, 2, 3, 1).contiguous()
            features = dev.feature_extractor((nhwc * 255).to(torch.uint8), nhwc)
        return self._rows(dev, features)

    def train_step(self, images, references, features=None, masks=None):
        dev = get_device(self._index)
        x = _image_batch(dev, images).contiguous()
        ref = _loss_reference(dev, x, references)
        rows = self._features(dev, x, features)
        if rows.shape[0] != x.shape[0]:
            raise ValueError(f"{rows.shape[0]} feature rows for {x.shape[0]} images")
        if masks is not None:
            masks = dev.tensor(np.asarray(masks)) if not isinstance(masks, torch.Tensor) else masks.to(dev.torch_device)
            want = (1 + 2 * self.num_blocks, int(rows.shape[0]), self.hidden_dim)
            if tuple(masks.shape) != want:
                raise ValueError(f"masks of shape {tuple(masks.shape)}, expected {want}")
            masks = (masks != 0).to(torch.uint8).contiguous()
        ws = dev.mlp_train_workspace(rows.shape[0], self.hidden_dim, self.num_blocks)
        cols = dev.mlp_train_forward(self._handle, rows, ws, self.dropout, masks, self.seed)
        _, saved, buf = dev.ref_loss_f32(_lib.LOSS_GATED, x, cols, ref, True, status=True)
        _, grad_cols = dev.ref_loss_bwd_f32(_lib.LOSS_GATED, x, cols, saved, ref, self._grad_loss, True, want_img=False)
        dev.mlp_backward(self._handle, rows, ws, grad_cols)
        dev.mlp_adam_step(self._handle, self.lr, self.betas, self.eps, self.max_norm)
        l1, l2 = _read_loss(dev, buf, x, cols)
        return float(np.float32(0.5) * np.float32(l1) + np.float32(0.5) * np.float32(l2)), {"l1": l1, "l2": l2}

    def validate_batch(self, images, references, features=None):
        """``validate``'s loop body (:316-329): ``(loss, {'l1', 'l2'})`` of the current weights in eval mode, one host read."""
        dev = get_device(self._index)
        x = _image_batch(dev, images)
        with torch.no_grad():
            cols = self.param_predictor.columns(self._features(dev, x, features), dev)
            _, parts = self.criterion.through(self.enhancement, x, GatedEnhancementPredictor._dict(cols), references)
        return float(np.float32(0.5) * np.float32(parts["l1"]) + np.float32(0.5) * np.float32(parts["l2"])), parts

    @staticmethod
    def _average(results):
        """(:303-306, :331-334) the averages over the batches"""
        results = list(results)
        n = len(results)
        total = sum(loss for loss, _ in results)
        parts = {k: sum(p[k] for _, p in results) / n for k in ("l1", "l2")}
        return total / n, parts

    def train_epoch(self, batches):
        return self._average(self.train_step(b["image"], b["reference"], b.get("features")) for b in batches)

    def validate(self, batches):
        return self._average(self.validate_batch(b["image"], b["reference"], b.get("features")) for b in batches)


QUALITY_KEYS = ("contrast", "sharpness", "entropy", "saturation", "brightness", "edge_density", "colorfulness", "naturalness")


class QualityAssessment:
    """Mirror of ``quality_assessment.QualityAssessment.comprehensive_assessment`` (quality_assessment.py:215-286)."""

    device: int | None = None

    @classmethod
    def comprehensive_assessment(cls, img, weights=None):
        """``img``: HxWx3 RGB float in [0, 1] -> ``(total_score, scores_dict)`` like the reference."""
        x = np.asarray(img)
        if x.ndim != 3 or x.shape[2] != 3:
            raise ValueError(f"expected an HxWx3 image, got {x.shape}")
        dev = get_device(cls.device)
        u8 = (x * 255).astype(np.uint8)  # quality_assessment.py:25 etc.: every score starts from this frame
        w = [weights.get(k, 0) for k in QUALITY_KEYS] if weights is not None else None
        row = dev.quality_scores(dev.tensor(u8[None]), dev.tensor(np.ascontiguousarray(x[None], dtype=np.float32)), w)
        row = row[0].cpu().numpy()
        return float(row[8]), {k: float(row[i]) for i, k in enumerate(QUALITY_KEYS)}


def quality_scores(frames_u8, frames_f32=None, weights=None, device: int | None = None):
    """Batch form on device or host arrays: ``[B,H,W,3]`` uint8 (and optionally the float32 images) -> ``[B,9]`` float64
    (eight scores in ``QUALITY_KEYS`` order, then the weighted total): best-of-N selection without leaving the GPU."""
    dev = get_device(device)
    batch, was_numpy, single = _as_batch_u8(frames_u8, dev)
    f32 = None
    if frames_f32 is not None:
        f32 = frames_f32 if hasattr(frames_f32, "data_ptr") else dev.tensor(np.ascontiguousarray(frames_f32, dtype=np.float32))
        if f32.dim() == 3:
            f32 = f32[None]
    w = [weights.get(k, 0) for k in QUALITY_KEYS] if isinstance(weights, dict) else weights
    return _finish(dev.quality_scores(batch, f32, w), was_numpy, single)


# config.py:28-75 (Config.STRATEGIES) and :77-84 (Config.QUALITY_WEIGHTS): the parameter sets and weights main.py labels with
CONFIG_STRATEGIES = {
    "strong_dehazing": {"name": "StrongDehazing", "omega": 0.5, "guided_radius": 15, "L_low": 10, "L_high": 95, "gamma": 1.2,
                        "apply_gamma": True},
    "medium_dehazing": {"name": "MediumDehazing", "omega": 0.6, "guided_radius": 20, "L_low": 15, "L_high": 92, "apply_gamma": True},
    "light_enhancement": {"name": "LightEnhancement", "omega": 0.4, "guided_radius": 10, "L_low": 15, "L_high": 95,
                          "apply_gamma": False},
    "clahe_enhancement": {"name": "CLAHEEnhancement", "clip_limit": 2.0, "tile_grid_size": (8, 8), "apply_gamma": False},
    "histogram_equalization": {"name": "HistogramEqualization", "L_low": 10, "L_high": 95},
}
CONFIG_QUALITY_WEIGHTS = {"contrast": 0.25, "sharpness": 0.20, "entropy": 0.15, "saturation": 0.15, "brightness": 0.15,
                          "edge_density": 0.10}


def _dict_params(dev, name, params):
    """uwie_params of apply_strategy(img, name, params) (ES:350-474: the keys a strategy reads, its in-code defaults otherwise)."""
    over = {}
    for key, field in (("omega", "omega"), ("guided_radius", "gf_ksize"), ("L_low", "L_low"), ("L_high", "L_high"),
                       ("clip_limit", "clip_limit"), ("gamma", "gamma")):
        if key in params:
            over[field] = params[key]
    if "tile_grid_size" in params:
        over["tiles_x"], over["tiles_y"] = (int(v) for v in params["tile_grid_size"])
    over["apply_gamma"] = int(bool(params.get("apply_gamma", False)))
    if "dark_patch" in params:  # (no key of the reference's: uwie_params.dark_patch, the dehazing strategies read it)
        over["dark_patch"] = int(params["dark_patch"])
    return dev.params(_lib.SURFACE_DICT, _lib.DICT_STRATEGIES[name], **over)


def select_best(frames, strategies=None, weights=None, device: int | None = None, return_all: bool = False,
                dark_patch: int | None = None, gray_world=None):
    """The labelling loop of ``SelfSupervisedSystem.build_dataset`` (main.py:118-146) for one frame or a batch, in ONE device
    call: every entry of ``strategies`` (default ``Config.STRATEGIES``, config.py:28-75: ``{key: {'name': ..., params}}``) goes
    through ``apply_strategy``, ``comprehensive_assessment`` with ``weights`` (default ``Config.QUALITY_WEIGHTS``) scores each
    result, and the first maximum wins (main.py:145).  The three dehazing strategies share one atmospheric-light quadtree.

    ``frames``: uint8 ``[H,W,3]`` / ``[B,H,W,3]`` (main.py:108 makes ``u8.astype(float32) / 255`` of exactly these).
    Returns ``(best_names, best_images, scores)``: the winner's ``'name'`` per frame (a string for a single frame), its
    ``(enhanced * 255).astype(uint8)`` image (main.py:154-155 writes that), and ``scores[frame][name] = total``; with
    ``return_all`` a fourth value ``{name: uint8 batch}`` holds every strategy's output.  A strategy the device cannot
    run fails the call: fall back to ``EnhancementStrategies.apply_strategy`` + ``QualityAssessment`` per strategy, whose
    ``try`` blocks give a failing strategy the score 0.0 like main.py:139-142.

    ``dark_patch`` (optional): uwie_params.dark_patch of every dehazing entry whose own dict has no ``'dark_patch'`` key.
    ``gray_world`` (``True`` or a dict of ``red`` / ``blue`` / ``max_gain``): every strategy starts from ``gray_world(frames)``.
    """
    strategies = CONFIG_STRATEGIES if strategies is None else strategies
    if dark_patch is not None:
        strategies = {k: ({"dark_patch": int(dark_patch), **v} if _lib.DICT_STRATEGIES.get(k, 9) <= 2 else v)
                      for k, v in strategies.items()}
    weights = CONFIG_QUALITY_WEIGHTS if weights is None else weights
    dev = get_device(device)
    batch, was_numpy, single = _as_balanced_batch_u8(frames, dev, gray_world)
    keys = list(strategies)
    for k in keys:
        if k not in _lib.DICT_STRATEGIES:
            raise ValueError(f"未知策略: {k}")
    plist = [_dict_params(dev, k, strategies[k]) for k in keys]
    names = [strategies[k].get("name", k) for k in keys]
    w = [weights.get(k, 0) for k in QUALITY_KEYS]
    best, img, scores, every = dev.select_best_u8(batch, plist, w, want_all=return_all)
    best_h = best.cpu().tolist()
    tot = scores[:, :, 8].cpu().numpy()
    dev.check_status()
    best_names = [names[i] for i in best_h]
    table = [{names[k]: float(tot[k, b]) for k in range(len(keys))} for b in range(len(best_h))]
    out = (best_names[0] if single else best_names, _finish(img, was_numpy, single), table[0] if single else table)
    if return_all:
        out = out + ({names[k]: _finish(every[k], was_numpy, single) for k in range(len(keys))},)
    return out


# include/uwie.h uwie_underwater_scores_u8: the columns of a row of underwater scores
UNDERWATER_SCORE_NAMES = ("sigma_c", "con_l", "mu_s", "uciqe", "uicm", "uism", "uiconm", "uiqm")


def underwater_scores(frames, device: int | None = None):
    """UCIQE, UIQM and their parts in the fixed form include/uwie.h states (an extension without a reference counterpart), on
    the device: uint8 ``[H,W,3]`` / ``[B,H,W,3]``, NumPy or a torch ROCm tensor -> float64 ``(8,)`` / ``(B, 8)`` of the same
    kind, columns in ``UNDERWATER_SCORE_NAMES`` order."""
    dev = get_device(device)
    batch, was_numpy, single = _as_batch_u8(frames, dev)
    return _finish(dev.underwater_scores(batch), was_numpy, single, dev)


class UnderwaterQuality:
    """UCIQE / UIQM of one image: a uint8 RGB frame, or a float image in [0, 1] quantised with ``(x * 255).astype(uint8)``
    like every score of ``QualityAssessment``."""

    device: int | None = None

    @classmethod
    def scores(cls, img) -> dict:
        """``{name: value}`` for every entry of ``UNDERWATER_SCORE_NAMES``."""
        x = np.asarray(img.cpu() if hasattr(img, "data_ptr") else img)
        if x.ndim != 3 or x.shape[2] != 3:
            raise ValueError(f"expected an HxWx3 image, got {x.shape}")
        u8 = x if x.dtype == np.uint8 else (x * 255).astype(np.uint8)
        row = underwater_scores(np.ascontiguousarray(u8), device=cls.device)
        return {k: float(row[i]) for i, k in enumerate(UNDERWATER_SCORE_NAMES)}

    @classmethod
    def uciqe(cls, img) -> float:
        return cls.scores(img)["uciqe"]

    @classmethod
    def uiqm(cls, img) -> float:
        return cls.scores(img)["uiqm"]


def select_best_underwater(frames, strategies=None, metric: str = "uiqm", device: int | None = None, return_all: bool = False,
                           gray_world=None):
    """``select_best``'s labelling loop with the winner picked by an underwater metric instead of the weighted total: every
    entry of ``strategies`` (default ``Config.STRATEGIES``; a dict like ``select_best``'s, or a list of ``(key, params)`` pairs,
    which can name a key more than once) is applied to the frames (uwie_select_best_u8 with its outputs kept), the n * B results are scored in one uwie_underwater_scores_u8 call, and per frame the first maximum of ``metric``
    (``"uiqm"`` or ``"uciqe"``) in the strategies' order wins (uwie_pick_best_u8).  Nothing comes back to the host in between.

    Returns ``(best_names, best_images, scores)``: the winner's ``'name'`` per frame (a string for a single frame), its uint8
    image, and ``scores`` shaped ``(n, B, 8)`` (B = 1 for a single frame) in ``UNDERWATER_SCORE_NAMES`` order, the sets in
    ``strategies``' order; with ``return_all`` a fourth value ``{name: uint8 batch}`` holds every strategy's output.
    ``gray_world``: as for ``select_best``."""
    if metric not in ("uiqm", "uciqe"):
        raise ValueError(f"metric must be 'uiqm' or 'uciqe', got {metric!r}")
    strategies = CONFIG_STRATEGIES if strategies is None else strategies
    sets = list(strategies.items()) if isinstance(strategies, dict) else [(k, dict(v)) for k, v in strategies]
    dev = get_device(device)
    batch, was_numpy, single = _as_balanced_batch_u8(frames, dev, gray_world)
    for k, _ in sets:
        if k not in _lib.DICT_STRATEGIES:
            raise ValueError(f"未知策略: {k}")
    plist = [_dict_params(dev, k, v) for k, v in sets]
    names = [v.get("name", k) for k, v in sets]
    _, _, _, every = dev.select_best_u8(batch, plist, None, want_all=True)
    n, B, H, W = (int(v) for v in every.shape[:4])
    scores = dev.underwater_scores(every.view(n * B, H, W, 3), gray_shift=plist[0].gray_shift).view(n, B, len(UNDERWATER_SCORE_NAMES))
    best, img = dev.pick_best_u8(scores, UNDERWATER_SCORE_NAMES.index(metric), every)
    best_h = best.cpu().tolist()
    dev.check_status()
    best_names = [names[i] for i in best_h]
    out = (best_names[0] if single else best_names, _finish(img, was_numpy, single), scores.cpu().numpy() if was_numpy else scores)
    if return_all:
        out = out + ({names[k]: _finish(every[k], was_numpy, single) for k in range(len(sets))},)
    return out


# include/uwie.h uwie_reference_scores_u8: the columns of a row of full-reference scores
REFERENCE_SCORE_NAMES = ("mae", "mse", "psnr", "ssim_y", "ssim_r", "ssim_g", "ssim_b", "ssim_rgb")


def _refs_for(refs, batch, dev: Device):
    """The references of a batch [B,H,W,3] on the device: B of them, or one (a frame or a batch of 1) for all."""
    r, _, _ = _as_batch_u8(refs, dev)
    if tuple(r.shape[1:]) != tuple(batch.shape[1:]):
        raise ValueError(f"references are {tuple(r.shape[1:])}, frames {tuple(batch.shape[1:])}")
    if r.shape[0] not in (1, batch.shape[0]):
        raise ValueError(f"{r.shape[0]} references for {batch.shape[0]} frames: give one per frame, or one for all")
    return r


def reference_scores(frames, refs, device: int | None = None):
    """MAE, MSE, PSNR and SSIM (11 x 11 Gaussian window, valid windows; include/uwie.h states the definition) of results against
    their references, on the device: uint8 ``[H,W,3]`` / ``[B,H,W,3]``, NumPy or a torch ROCm tensor; ``refs`` of the same
    shape, or a single frame / a batch of 1 compared with every frame -> float64 ``(8,)`` / ``(B, 8)`` of the same kind as
    ``frames``, columns in ``REFERENCE_SCORE_NAMES`` order.  Frames below 11 x 11 have no window: their SSIM columns are NaN."""
    dev = get_device(device)
    batch, was_numpy, single = _as_batch_u8(frames, dev)
    return _finish(dev.reference_scores(batch, _refs_for(refs, batch, dev)), was_numpy, single, dev)


class ReferenceQuality:
    """PSNR / SSIM of one image against its reference: uint8 RGB frames, or float images in [0, 1] quantised with
    ``(x * 255).astype(uint8)`` like ``UnderwaterQuality``."""

    device: int | None = None

    @staticmethod
    def _u8(img):
        x = np.asarray(img.cpu() if hasattr(img, "data_ptr") else img)
        if x.ndim != 3 or x.shape[2] != 3:
            raise ValueError(f"expected an HxWx3 image, got {x.shape}")
        return np.ascontiguousarray(x if x.dtype == np.uint8 else (x * 255).astype(np.uint8))

    @classmethod
    def scores(cls, img, ref) -> dict:
        """``{name: value}`` for every entry of ``REFERENCE_SCORE_NAMES``."""
        row = reference_scores(cls._u8(img), cls._u8(ref), device=cls.device)
        return {k: float(row[i]) for i, k in enumerate(REFERENCE_SCORE_NAMES)}

    @classmethod
    def psnr(cls, img, ref) -> float:
        return cls.scores(img, ref)["psnr"]

    @classmethod
    def ssim(cls, img, ref, channels: str = "y") -> float:
        """SSIM of the gray planes (``"y"``) or the mean of the three channels' (``"rgb"``)."""
        if channels not in ("y", "rgb"):
            raise ValueError(f"channels must be 'y' or 'rgb', got {channels!r}")
        return cls.scores(img, ref)["ssim_" + channels]


def select_best_reference(frames, refs, strategies=None, metric: str = "ssim_y", device: int | None = None, return_all: bool = False,
                          gray_world=None):
    """``select_best_underwater``'s labelling loop with the winner picked by closeness to a ground truth: every entry of
    ``strategies`` (default ``Config.STRATEGIES``; a dict, or a list of ``(key, params)`` pairs) is applied to the frames, the
    n * B results are scored against the B references in one uwie_reference_scores_u8 call (``ref_batch = B``: no copies of
    the references), and per frame the first maximum of ``metric`` (``"psnr"``, ``"ssim_y"`` or ``"ssim_rgb"``, the columns
    where larger is better) in the strategies' order wins (uwie_pick_best_u8).  ``refs``: one reference per frame, or one for all.

    Returns ``(best_names, best_images, scores)`` like ``select_best_underwater``, ``scores`` shaped ``(n, B, 8)`` in
    ``REFERENCE_SCORE_NAMES`` order; with ``return_all`` a fourth value ``{name: uint8 batch}`` holds every strategy's output.
    ``gray_world``: as for ``select_best`` (the frames are balanced, the references are not)."""
    if metric not in ("psnr", "ssim_y", "ssim_rgb"):
        raise ValueError(f"metric must be 'psnr', 'ssim_y' or 'ssim_rgb', got {metric!r}")
    strategies = CONFIG_STRATEGIES if strategies is None else strategies
    sets = list(strategies.items()) if isinstance(strategies, dict) else [(k, dict(v)) for k, v in strategies]
    dev = get_device(device)
    batch, was_numpy, single = _as_balanced_batch_u8(frames, dev, gray_world)
    r = _refs_for(refs, batch, dev)
    for k, _ in sets:
        if k not in _lib.DICT_STRATEGIES:
            raise ValueError(f"未知策略: {k}")
    plist = [_dict_params(dev, k, v) for k, v in sets]
    names = [v.get("name", k) for k, v in sets]
    _, _, _, every = dev.select_best_u8(batch, plist, None, want_all=True)
    n, B, H, W = (int(v) for v in every.shape[:4])
    scores = dev.reference_scores(every.view(n * B, H, W, 3), r, gray_shift=plist[0].gray_shift).view(n, B, len(REFERENCE_SCORE_NAMES))
    best, img = dev.pick_best_u8(scores, REFERENCE_SCORE_NAMES.index(metric), every)
    best_h = best.cpu().tolist()
    dev.check_status()
    best_names = [names[i] for i in best_h]
    out = (best_names[0] if single else best_names, _finish(img, was_numpy, single), scores.cpu().numpy() if was_numpy else scores)
    if return_all:
        out = out + ({names[k]: _finish(every[k], was_numpy, single) for k in range(len(sets))},)
    return out


def extract_all_features(img, device: int | None = None):
    """``vgg_16_UIE.extract_all_features(img)`` (vgg_16_UIE.py:435-466) for a uint8 RGB frame ``[H,W,3]`` (returns the
    reference's ``(79,)`` float32 vector) or a batch ``[B,H,W,3]`` (returns ``(B, 79)``).  Float inputs of the reference
    (``_ensure_float01``) are not taken here: pass the decoded uint8 frame."""
    dev = get_device(device)
    if not hasattr(img, "data_ptr") and np.asarray(img).dtype != np.uint8:
        raise ValueError("extract_all_features on the device takes uint8 frames")
    batch, was_numpy, single = _as_batch_u8(img, dev)
    return _finish(dev.extract_features_u8(batch), was_numpy, single)


# feature_extraction.FeatureExtractor (feature_extraction.py:13-295): the classifier input of main.py:116,420
FEATURE_EXTRACTOR_KEYS = (
    [f"lab_{c}_{s}" for c in "Lab" for s in ("mean", "std", "skew", "kurtosis")]
    + [f"hsv_{c}_{s}" for c in "HSV" for s in ("mean", "std")]
    + ["ccf", "ccf_M", "ccf_D", "lab_a_mean_ccf", "lab_b_mean_ccf"]
    + [f"rgb_{c}_{s}" for c in "RGB" for s in ("mean", "std", "min", "max")]
    + [f"lbp_{i}" for i in range(10)]
    + [f"glcm_{p}_{s}" for p in ("contrast", "dissimilarity", "homogeneity", "energy", "correlation", "ASM") for s in ("mean", "std")]
    + ["dct_low", "dct_mid", "dct_high", "dct_abs_mean", "dct_abs_std"]
    + ["sobel_mean", "sobel_std", "sobel_max", "canny_density", "laplacian_abs_mean", "laplacian_std", "laplacian_var"]
    + ["gray_std", "gray_entropy", "gray_mean", "gray_median", "gray_p25", "gray_p75", "gray_range", "sat_mean", "sat_std",
       "rms_contrast"])
_FX_GROUPS = {"color": (0, 35), "texture": (35, 57), "frequency": (57, 62), "edge": (62, 69), "quality": (69, 79)}


def feature_extractor_keys(H: int, W: int):
    """Names of the values ``extract_all_features`` returns for an HxW frame (the DCT block is absent when H or W is odd > 1)."""
    if _lib.load().uwie_feature_extractor_count(int(H), int(W)) == 79:
        return list(FEATURE_EXTRACTOR_KEYS)
    return FEATURE_EXTRACTOR_KEYS[:57] + FEATURE_EXTRACTOR_KEYS[62:]


def feature_extractor_rows(frames, frames_f32=None, device: int | None = None):
    """``FeatureExtractor.extract_all_features`` for a batch in one device call: ``[B,H,W,3]`` uint8 (NumPy or a ROCm tensor)
    -> ``[B,79]`` float64 (``[B,74]`` when H or W is odd and > 1); a single ``[H,W,3]`` frame gives one row.  ``frames_f32``
    (optional, float32, same shape): the float images the frames were quantised from, read by the RGB block (indices 23-34)."""
    dev = get_device(device)
    batch, was_numpy, single = _as_batch_u8(frames, dev)
    f32 = None
    if frames_f32 is not None:
        f32 = frames_f32 if hasattr(frames_f32, "data_ptr") else dev.tensor(np.ascontiguousarray(frames_f32, dtype=np.float32))
        if f32.dim() == 3:
            f32 = f32[None]
    out = dev.feature_extractor(batch, f32)
    dev.check_status()
    return _finish(out, was_numpy, single)


class FeatureExtractor:
    """Mirror of ``feature_extraction.FeatureExtractor`` (feature_extraction.py:13-295) on the device.  Every method takes an
    HxWx3 RGB image, float in [0, 1] like the reference, or a uint8 frame (then the float image is ``u8 / 255``), and
    returns a float64 vector; ``extract_all_features`` has 79 values (74 when H or W is odd and > 1: the reference's
    ``cv2.dct`` refuses odd sizes and its ``try`` drops that block).  The group methods are slices of the same device call;
    ``extract_frequency_features`` raises ``ValueError`` for odd sizes, as the reference's does."""

    device: int | None = None

    @classmethod
    def _row(cls, img):
        x = np.asarray(img)
        if x.ndim != 3 or x.shape[2] != 3:
            raise ValueError(f"expected an HxWx3 image, got {x.shape}")
        if x.size == 0:
            raise ValueError("empty image")
        if x.dtype == np.uint8:
            return feature_extractor_rows(x, device=cls.device)
        if x.dtype.kind != "f":
            raise TypeError(f"expected a float image in [0, 1] or uint8, got {x.dtype}")
        if not (np.all(x >= 0) and np.all(x <= 1)):  # (NaN fails both)
            raise ValueError("float image values must lie in [0, 1]")
        u8 = (x * 255).astype(np.uint8)  # feature_extraction.py:30,89,134,176,215
        if x.dtype == np.float32 and np.array_equal(u8.astype(np.float32) / _F255, x):
            return feature_extractor_rows(u8, device=cls.device)  # u8-derived: its RGB block is the u8 frame's, exactly
        return feature_extractor_rows(u8, np.ascontiguousarray(x, dtype=np.float32), device=cls.device)

    @classmethod
    def _group(cls, img, name):
        row = cls._row(img)
        lo, hi = _FX_GROUPS[name]
        if row.size == 74:
            if name == "frequency":
                raise ValueError("Odd-size DCT's are not implemented")
            if lo >= 62:
                lo, hi = lo - 5, hi - 5
        return row[lo:hi]

    @classmethod
    def extract_color_features(cls, img):
        return cls._group(img, "color")

    @classmethod
    def extract_texture_features(cls, img):
        return cls._group(img, "texture")

    @classmethod
    def extract_frequency_features(cls, img):
        return cls._group(img, "frequency")

    @classmethod
    def extract_edge_features(cls, img):
        return cls._group(img, "edge")

    @classmethod
    def extract_quality_features(cls, img):
        return cls._group(img, "quality")

    @classmethod
    def extract_all_features(cls, img):
        return cls._row(img)


# ------------------------------------------------------------------ trainer / predictor input batches (cv2.resize on the device)
IMAGENET_MEAN = (0.485, 0.456, 0.406)  # vgg_16_UIE.py:327-330, use_trained_model.py:35-36 (T.Normalize)
IMAGENET_STD = (0.229, 0.224, 0.225)


def _frame_set(frames, dev: Device):
    """One frame, a batch or a ragged list -> (what Device.resize_rgb takes, was_numpy, single, sizes)."""
    if isinstance(frames, (list, tuple)):
        if not frames:
            raise ValueError("empty frame list")
        was_numpy = isinstance(frames[0], np.ndarray)
        items = [np.ascontiguousarray(f) if isinstance(f, np.ndarray) else f.to(dev.torch_device).contiguous() for f in frames]
        return items, was_numpy, False, [(int(f.shape[0]), int(f.shape[1])) for f in items]
    batch, was_numpy, single = _as_batch_u8(frames, dev)
    return batch, was_numpy, single, [(int(batch.shape[1]), int(batch.shape[2]))] * int(batch.shape[0])


def _dsize(dsize):
    w, h = (int(v) for v in dsize)
    if w < 1 or h < 1:
        raise ValueError(f"dsize must be positive (width, height), got {tuple(dsize)}")
    return h, w


def _norm_arg(normalize):
    if normalize is None:
        return None
    if isinstance(normalize, str):
        if normalize != "imagenet":
            raise ValueError(f"unknown normalisation {normalize!r}")
        return IMAGENET_MEAN, IMAGENET_STD
    mean, std = normalize
    if len(mean) != 3 or len(std) != 3:
        raise ValueError("normalize: (mean, std) with three values each")
    return tuple(float(v) for v in mean), tuple(float(v) for v in std)


def resize_frames(frames, dsize, flips=None, device: int | None = None):
    """``cv2.resize(frame, dsize)`` (INTER_LINEAR) of uint8 RGB frames on the device: one ``[H,W,3]`` frame, a ``[B,H,W,3]``
    batch or a list of frames of any sizes, in one launch.  ``dsize`` is OpenCV's ``(width, height)``.  ``flips``: per-frame
    flags, 1 = ``np.fliplr`` and 2 = ``np.flipud`` of the result.  Returns uint8 ``[B,h,w,3]`` (``[h,w,3]`` for one frame);
    NumPy in gives NumPy out, device tensors stay on the device.  The arithmetic is OpenCV's fixed-point path (DESIGN.md
    section 11)."""
    dev = get_device(device)
    h, w = _dsize(dsize)
    src, was_numpy, single, _ = _frame_set(frames, dev)
    u8, _, _ = dev.resize_rgb(src, h, w, flips=flips)
    out = _finish(u8, was_numpy, single, dev)
    if not was_numpy:
        dev.check_status()
    return out


def image_tensor(frames, dsize=None, normalize=None, flips=None, device: int | None = None):
    """Float32 ``[B,3,h,w]`` on the device from uint8 RGB frames: ``u8.astype(float32) / 255.0`` then ``permute(2, 0, 1)``,
    after ``cv2.resize(frame, dsize)`` when ``dsize`` is given (frames may then differ in size).  ``dsize=None`` keeps the
    full resolution, as ``EnhancementPredictor._img_to_tensor`` (use_trained_model.py:48-51) does (frames of one size).
    ``normalize``: ``"imagenet"`` or ``(mean, std)`` applies torchvision's ``Normalize`` (float32 ``sub`` then ``div``)."""
    dev = get_device(device)
    src, _, _, sizes = _frame_set(frames, dev)
    if dsize is None:
        if len(set(sizes)) != 1:
            raise ValueError("frames of different sizes need a dsize")
        h, w = sizes[0]
    else:
        h, w = _dsize(dsize)
    norm = _norm_arg(normalize)
    _, f32, nrm = dev.resize_rgb(src, h, w, flips=flips, want_u8=False, want_f32=norm is None, norm=norm)
    dev.check_status()
    return f32 if norm is None else nrm


def vgg_input(frames, size: int = 224, device: int | None = None):
    """``EnhancementPredictor._preprocess_for_vgg`` (use_trained_model.py:39-46) for uint8 RGB frames, batched: resize to
    ``size`` x ``size``, ``/ 255``, CHW, ImageNet ``Normalize``.  Returns float32 ``[B,3,size,size]`` on the device.  (The
    reference quantises its float image with ``(img * 255).astype(uint8)``; for ``u8 / 255`` that gives the frame back.)"""
    return image_tensor(frames, (size, size), normalize="imagenet", device=device)


def _draw_flips(n: int):
    """augment_pair's draws (vgg_16_UIE.py:344-356), per item in index order: horizontal first, then vertical."""
    out = np.zeros(n, np.uint8)
    for i in range(n):
        if np.random.rand() > 0.5:
            out[i] |= _lib.FLIP_LR
        if np.random.rand() > 0.5:
            out[i] |= _lib.FLIP_UD
    return out


def training_batch(images, references=None, size: int = 256, features="extractor", augment: bool = False, flips=None,
                   device: int | None = None):
    """A training batch on the device, as the reference's data loaders collate it from their datasets' items:
    ``{'image', 'reference'}`` float32 ``[B,3,size,size]`` and ``'features'`` float32 ``[B,F]``.

    ``images``: uint8 RGB frames (a ``[B,H,W,3]`` batch or a list of frames of any sizes, NumPy or device tensors).
    ``references``: None, or one entry per image (a frame, or None for a missing reference: the reference is then the
    image, ``ref = img.copy()``).  An image and its reference may differ in size; each is resized on its own.
    Per frame: ``cv2.resize(frame, (size, size))``, ``astype(float32) / 255.0``, CHW -- in one launch for images and
    references together.
    ``features``: ``"extractor"`` -- ``EnhancementDataset`` (deep_learning_parameters.py:214-247, size 256):
    ``FeatureExtractor.extract_all_features`` of the resized image (``feature_extractor_rows``, cast to float32);
    ``"basic"`` -- ``ImprovedEnhancementDataset`` (vgg_16_UIE.py:335-422, size 224): ``extract_basic_features`` of the
    (flipped) resized image (``uwie_extract_features_u8``); ``None``: zeros ``[B,79]``.  Features describe the image as
    the batch holds it, flipped when it is flipped.
    ``augment``: draw each item's flips from ``np.random`` as ``augment_pair`` does (horizontal then vertical, items in
    index order), so a seeded ``np.random`` gives a single-process pass of the reference dataset.  ``flips`` (per-item
    flags, 1 = fliplr, 2 = flipud) overrides the draws.  Image and reference get the same flips."""
    if features not in ("extractor", "basic", None):
        raise ValueError(f"features must be 'extractor', 'basic' or None, got {features!r}")
    dev = get_device(device)
    src, _, _, sizes = _frame_set(images, dev)
    B = len(sizes)
    if flips is not None:
        fl = np.asarray(flips, dtype=np.int64).reshape(-1)
        if fl.size != B:
            raise ValueError(f"flips: {fl.size} values for {B} images")
    elif augment:
        fl = _draw_flips(B)
    else:
        fl = np.zeros(B, np.int64)
    refs = [None] * B if references is None else list(references)
    if len(refs) != B:
        raise ValueError(f"{len(refs)} references for {B} images")
    present = [i for i, r in enumerate(refs) if r is not None]
    frames = list(src) if isinstance(src, list) else [src[i] for i in range(B)]
    ref_frames = [np.ascontiguousarray(refs[i]) if isinstance(refs[i], np.ndarray) else refs[i].to(dev.torch_device).contiguous()
                  for i in present]
    if ref_frames and isinstance(frames[0], np.ndarray) != isinstance(ref_frames[0], np.ndarray):
        ref_frames = [f.cpu().numpy() if isinstance(frames[0], np.ndarray) else dev.tensor(f) for f in ref_frames]
    allf = np.concatenate([fl, fl[present]]) if present else fl
    u8, f32, _ = dev.resize_rgb(frames + ref_frames, size, size, flips=allf, want_u8=features is not None, want_f32=True)
    image = f32[:B]
    reference = image.clone()
    if present:
        reference[torch.as_tensor(present, device=dev.torch_device)] = f32[B:]
    if features == "extractor":
        feats = dev.feature_extractor(u8[:B]).to(torch.float32)
    elif features == "basic":
        feats = dev.extract_features_u8(u8[:B])
    else:
        feats = torch.zeros((B, 79), dtype=torch.float32, device=dev.torch_device)
    dev.check_status()
    return {"image": image, "reference": reference, "features": feats}


# ------------------------------------------------------------------ float <-> u8 bridging
def _recover_u8(img):
    """Invert ``u8.astype(float32)/255`` [+ ``color_correction``] exactly; returns (u8 frame, cast kind)."""
    x = np.asarray(img)
    if x.ndim != 3 or x.shape[2] != 3:
        raise ValueError(f"expected an HxWx3 image, got {x.shape}")
    if x.size == 0:
        raise ValueError("empty image")
    x32 = x.astype(np.float32)
    if x.dtype != np.float32 and not np.array_equal(x32.astype(x.dtype), x):
        raise UnsupportedInputError("float image is not float32-representable u8/255 data")
    table = np.arange(256, dtype=np.float32) / _F255
    for kind, chan in (("normal", None), ("greenish", 1), ("bluish", 2)):
        ok, u8 = True, np.empty(x.shape, np.uint8)
        for c in range(3):
            lut = table * _ATTEN if c == chan else table
            idx = np.clip(np.searchsorted(lut, x32[:, :, c]), 0, 255)
            if not np.array_equal(lut[idx], x32[:, :, c]):
                ok = False
                break
            u8[:, :, c] = idx
        if ok:
            return u8, kind
    raise UnsupportedInputError("float image is not u8-derived (u8/255, optionally colour-corrected): unsupported input")


def _float_kind(img):
    """'u8' for a u8 frame, 'derived' for a u8-derived float image, else the dtype name of a general float image."""
    x = np.asarray(img)
    if x.dtype == np.uint8:
        return "u8"
    try:
        _recover_u8(x)
        return "derived"
    except UnsupportedInputError:
        if x.dtype in (np.float32, np.float64):
            return x.dtype.name
        raise


def detect_image_type(img, device: int | None = None) -> str:
    """six_stadigy.py:292-302 on a float image (u8-derived: from its u8 frame; general float32: sequential mean on the
    device) or a u8 frame."""
    dev = get_device(device)
    what = _float_kind(img)
    if what == "float32":
        kind, _ = dev.cast_classify_f32(dev.tensor(np.ascontiguousarray(img)[None]))
        return _lib.CAST_KINDS[int(kind[0])]
    if what == "float64":
        raise UnsupportedInputError("detect_image_type: general float64 images are not supported (six_stadigy.py works on float32)")
    u8 = img if what == "u8" else _recover_u8(img)[0]
    kind, _ = dev.cast_classify(dev.tensor(u8[None]))
    return _lib.CAST_KINDS[int(kind[0])]


def color_correction(img, image_type: str, device: int | None = None):
    """six_stadigy.py:305-323.  ``"normal"`` returns the input object itself, like the reference."""
    if image_type not in ("greenish", "bluish"):
        return img
    dev = get_device(device)
    if _float_kind(img) == "float32":  # general float image
        k = torch.tensor([_lib.CAST_KINDS.index(image_type)], dtype=torch.int32, device=dev.torch_device)
        return dev.color_correct_f32(dev.tensor(np.ascontiguousarray(img)[None]), k)[0].cpu().numpy()
    u8, kind = _recover_u8(img)
    if kind != "normal":
        raise ValueError("image is already colour-corrected")
    k = torch.tensor([_lib.CAST_KINDS.index(image_type)], dtype=torch.int32, device=dev.torch_device)
    return dev.normalise_correct(dev.tensor(u8[None]), k)[0].cpu().numpy()


class SixStrategies:
    """Mirror of ``six_stadigy.EnhancementStrategies`` (strategy1..6: float32 HxWx3 in [0,1] -> float32 HxWx3)."""

    device: int | None = None
    dark_patch: int = 1  # uwie_params.dark_patch of strategies 1-3 (no reference counterpart above 1); u8-derived images only

    @classmethod
    def _run(cls, number, img):
        dev = get_device(cls.device)
        what = _float_kind(img)
        patch = int(cls.dark_patch) if number <= 3 else 1
        if patch > 1 and what in ("float32", "float64"):
            raise UnsupportedInputError("dark_patch > 1 is built for u8-derived images only: a general float image has no patched route")
        if what == "float32":  # general float image: strategyN(img) as it stands (no cast detection inside, S6:230-285)
            p = dev.params(_lib.SURFACE_SIX, number, cast_correct=0, forced_cast=-1)
            return dev.enhance_float(dev.tensor(np.ascontiguousarray(img)[None]), p)[1][0].cpu().numpy()
        if what == "float64":
            raise UnsupportedInputError("six_stadigy strategies take float32 images (six_stadigy.py:406); a general float64 image "
                                        "is only supported on the dict surface (EnhancementStrategies.apply_strategy)")
        u8, kind = _recover_u8(img)
        # a colour-corrected input is replayed on the device from its u8 frame through a forced cast kind
        p = dev.params(_lib.SURFACE_SIX, number, cast_correct=0, forced_cast=_lib.CAST_KINDS.index(kind) or -1, dark_patch=patch)
        _, outf = dev.enhance_u8(dev.tensor(u8[None]), p, want_float=True)
        return outf[0].cpu().numpy()

    @classmethod
    def strategy1_strong_dehazing(cls, img):
        return cls._run(1, img)

    @classmethod
    def strategy2_medium_dehazing(cls, img):
        return cls._run(2, img)

    @classmethod
    def strategy3_light_dehazing(cls, img):
        return cls._run(3, img)

    @classmethod
    def strategy4_clahe_enhancement(cls, img):
        return cls._run(4, img)

    @classmethod
    def strategy5_white_balance(cls, img):
        return cls._run(5, img)

    @classmethod
    def strategy6_histogram_eq(cls, img):
        return cls._run(6, img)


class EnhancementStrategies:
    """Mirror of ``enhancement_strategies.EnhancementStrategies.apply_strategy`` (ES:477-508)."""

    device: int | None = None
    swallow_errors = True  # ES:503-508 prints the failure and returns the input image

    @classmethod
    def apply_strategy(cls, img, strategy_name, params):
        if strategy_name not in _lib.DICT_STRATEGIES:
            raise ValueError(f"未知策略: {strategy_name}")
        try:
            return cls._run(img, strategy_name, params)
        except UnsupportedInputError:
            raise  # not a strategy failure: never handed back as if it had been processed
        except Exception as exc:  # noqa: BLE001 - mirrors the reference's blanket except
            if not cls.swallow_errors:
                raise
            print(f"策略 {strategy_name} 執行失敗: {exc}")
            return img

    @classmethod
    def _run(cls, img, name, params):
        dev = get_device(cls.device)
        x = np.asarray(img)
        if x.dtype not in (np.float32, np.float64):
            raise UnsupportedInputError(f"apply_strategy takes float32 / float64 images in [0, 1], got {x.dtype}")
        if x.ndim != 3 or x.shape[2] != 3 or x.size == 0:
            raise ValueError(f"expected a non-empty HxWx3 image, got {x.shape}")
        u8 = None
        if x.dtype == np.float32:  # main.py:108 hands over u8.astype(float32)/255: the fast path from the u8 frame
            try:
                cand, kind = _recover_u8(x)
                if kind == "normal":
                    u8 = cand
            except UnsupportedInputError:
                pass
        p = _dict_params(dev, name, params)
        if u8 is None and p.dark_patch > 1:
            raise UnsupportedInputError("dark_patch > 1 is built for u8-derived float32 images (u8 / 255) only: a general float image "
                                        "has no patched route")
        # float64 like the reference (ES:247,307,345): a caller's (enhanced * 255).astype(np.uint8) (main.py:155) then
        # truncates the same values as with the reference
        if u8 is not None:
            return dev.enhance_u8_f64(dev.tensor(u8[None]), p)[1][0].cpu().numpy()
        # any other float32 / float64 image (the reference's harness inputs are np.random.rand): general float path
        return dev.enhance_float(dev.tensor(np.ascontiguousarray(x)[None]), p)[1][0].cpu().numpy()
