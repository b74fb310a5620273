"""The gated-gamma DifferentiableEnhancement (deep_learning_parameters.py:24-90) on the device, forward and backward: against
the real module (tests/golden/dlp_grads.npz) and, at larger sizes, against the torch restatement (tests/dlp_grad_ref.py).
Tolerances: DESIGN.md section 10."""
import os

import numpy as np
import pytest

import dlp_grad_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dlp_grads.npz")
KEYS = ("L_low", "L_high", "use_gamma", "gamma")


@pytest.fixture(scope="module")
def dev():
    import underwater_image_enhancement_amd as uw

    return uw.get_device(0)


def golden_cases():
    with np.load(GOLDEN, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    tags = sorted({k.split("/")[0] for k in d} - {"errors"})
    return {t: {k.split("/", 1)[1]: v for k, v in d.items() if k.startswith(t + "/")} for t in tags}


def run_module(dev, img, par, grad_out, img_grad=True):
    """loss.backward() through uw.GatedDifferentiableEnhancement on device tensors -> (out, grad_img, {key: grad}, leaves)."""
    import torch

    import underwater_image_enhancement_amd as uw

    x = torch.from_numpy(np.ascontiguousarray(img)).to(dev.torch_device).requires_grad_(img_grad)
    leaves = {k: torch.from_numpy(np.asarray(par[k], np.float32)).to(dev.torch_device).requires_grad_(True) for k in KEYS}
    out = uw.GatedDifferentiableEnhancement()(x, leaves)
    assert out.grad_fn is not None
    (out * torch.from_numpy(np.asarray(grad_out, np.float32)).to(dev.torch_device)).sum().backward()
    assert leaves["L_low"].grad is None and leaves["L_high"].grad is None
    grads = {f"grad_{k}": leaves[k].grad.cpu().numpy() for k in ("use_gamma", "gamma")}
    return out.detach().cpu().numpy(), (x.grad.cpu().numpy() if img_grad else None), grads


def test_forward_matches_the_real_module(dev):
    import underwater_image_enhancement_amd as uw

    for tag, c in golden_cases().items():
        got = uw.GatedDifferentiableEnhancement()(c["img"], {k: c[k] for k in KEYS})
        assert isinstance(got, np.ndarray) and got.shape == c["out"].shape
        d = np.abs(got.astype(np.float64) - c["out"])
        assert (d <= 2.0**-23).all(), f"{tag}: forward off by {d.max():.3g}"
        u = c["use_gamma"].reshape(-1)
        for b in np.flatnonzero(u == 0):
            assert np.array_equal(got[b].view(np.int32), c["out"][b].view(np.int32)), f"{tag} image {b}: use_gamma = 0"


def test_gradients_match_the_real_module(dev):
    worst = 0.0
    for tag, c in golden_cases().items():
        _, gi, grads = run_module(dev, c["img"], c, c["grad_out"])
        want = {"grad_img": c["grad_img_stable"], "grad_use_gamma": c["grad_use_gamma"], "grad_gamma": c["grad_gamma"]}
        worst = max(worst, R.check_grads(c["img"], c["L_low"], c["L_high"], c["grad_out"], {"grad_img": gi, **grads}, want,
                                         tag=tag))
    print(f"worst grad_img error over the module's cases: {worst:.3f} of the bound")


def seeded(shape, rng, u8=False):
    if u8:
        return np.float32(rng.integers(0, 256, shape)) / np.float32(255.0)
    return rng.random(shape, dtype=np.float32)


@pytest.mark.parametrize("shape,u8,planar", [((4, 3, 256, 256), True, True), ((4, 3, 256, 256), False, False),
                                             ((2, 3, 1080, 1920), True, True), ((2, 3, 1080, 1920), False, False)])
def test_larger_cases_match_the_restatement(dev, shape, u8, planar):
    import underwater_image_enhancement_amd as uw

    rng = np.random.default_rng(sum(shape) * 7 + u8 * 3 + planar)
    B = shape[0]
    img = seeded(shape, rng, u8)
    if not planar:
        img = np.ascontiguousarray(img.transpose(0, 2, 3, 1))
    L_low = rng.uniform(5, 20, (B, 1)).astype(np.float32)
    L_high = rng.uniform(85, 98, (B, 1)).astype(np.float32)
    use = rng.uniform(0, 1, (B, 1)).astype(np.float32)
    gamma = rng.uniform(0.5, 3.0, (B, 1)).astype(np.float32)
    grad_out = rng.standard_normal(img.shape).astype(np.float32)
    _, want_img, want_u, want_g = R.grads(img, L_low, L_high, use, gamma, grad_out, planar=planar)
    x = dev.tensor(img).requires_grad_(True)
    p = dev.tensor(np.concatenate([L_low, L_high, use, gamma], axis=1)).requires_grad_(True)
    out = uw.GatedDiffEnhanceFunction.apply(x, p, planar, dev)
    out.backward(dev.tensor(grad_out))
    dev.check_status()
    gp = p.grad.cpu().numpy()
    assert not gp[:, :2].any()
    got = {"grad_img": x.grad.cpu().numpy(), "grad_use_gamma": gp[:, 2:3], "grad_gamma": gp[:, 3:4]}
    want = {"grad_img": want_img, "grad_use_gamma": want_u, "grad_gamma": want_g}
    w = R.check_grads(img, L_low, L_high, grad_out, got, want, planar=planar, tag=f"{shape} planar={planar}")
    print(f"{shape} u8={u8} planar={planar}: worst grad_img error {w:.3f} of the bound")


@pytest.mark.parametrize("planar", [True, False])
def test_forward_with_grad_is_the_inference_forward(dev, planar):
    import torch

    import underwater_image_enhancement_amd as uw

    rng = np.random.default_rng(5)
    img = rng.random((3, 3, 37, 53) if planar else (3, 37, 53, 3), dtype=np.float32)
    p = np.concatenate([rng.uniform(1, 30, (3, 1)), rng.uniform(65, 99, (3, 1)), np.array([[0.0], [1.0], [0.37]]),
                        rng.uniform(0.5, 3.0, (3, 1))], axis=1).astype(np.float32)
    want = dev.diff_gated_f32(dev.tensor(img), dev.tensor(p), planar)
    got = uw.GatedDiffEnhanceFunction.apply(dev.tensor(img).requires_grad_(True), dev.tensor(p), planar, dev)
    assert got.grad_fn is not None
    assert torch.equal(got.detach().view(torch.int32), want.view(torch.int32))
    if planar:  # the public class: grad path and inference path
        par = {k: torch.from_numpy(p[:, i:i + 1].copy()).to(dev.torch_device) for i, k in enumerate(KEYS)}
        with torch.no_grad():
            inf = uw.GatedDifferentiableEnhancement()(dev.tensor(img), par)
        par["gamma"].requires_grad_(True)
        trn = uw.GatedDifferentiableEnhancement()(dev.tensor(img), par)
        assert inf.grad_fn is None and trn.grad_fn is not None
        assert torch.equal(trn.detach().view(torch.int32), inf.view(torch.int32))
        assert torch.equal(inf.view(torch.int32), want.view(torch.int32))


def test_backward_is_deterministic(dev):
    c = golden_cases()["u8ties_2x3x24x31"]
    rng = np.random.default_rng(9)
    img = seeded((4, 3, 256, 256), rng, u8=True)
    par = {"L_low": np.full((4, 1), 3.0, np.float32), "L_high": np.full((4, 1), 97.0, np.float32),
           "use_gamma": rng.uniform(0, 1, (4, 1)).astype(np.float32), "gamma": rng.uniform(1.0, 1.5, (4, 1)).astype(np.float32)}
    grad_out = rng.standard_normal(img.shape).astype(np.float32)
    runs = [run_module(dev, img, par, grad_out) for _ in range(2)] + [run_module(dev, c["img"], c, c["grad_out"]) for _ in range(2)]
    for a, b in ((runs[0], runs[1]), (runs[2], runs[3])):
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32))
        assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
        for k in a[2]:
            assert np.array_equal(a[2][k].view(np.int32), b[2][k].view(np.int32)), k


def test_unindexable_positions_raise_and_the_device_carries_on(dev):
    import torch

    import underwater_image_enhancement_amd as uw
    from underwater_image_enhancement_amd import _lib

    rng = np.random.default_rng(3)
    img = rng.random((2, 3, 8, 8), dtype=np.float32)
    enh = uw.GatedDifferentiableEnhancement()
    good = {"L_low": [[5.0], [10.0]], "L_high": [[95.0], [90.0]], "use_gamma": [[0.4], [0.7]], "gamma": [[1.2], [1.4]]}
    want = enh(img, good)
    with pytest.raises(IndexError, match="index 64 is out of bounds"):
        enh(img, {**good, "L_high": [[95.0], [100.0]]})
    with pytest.raises(ValueError):
        enh(img, {**good, "L_low": [[np.nan], [10.0]]})
    with pytest.raises(OverflowError):
        enh(img, {**good, "L_low": [[5.0], [np.inf]]})
    g = torch.tensor([[1.2], [1.4]], device=dev.torch_device, requires_grad=True)
    with pytest.raises(IndexError):
        enh(dev.tensor(img), {**good, "L_low": [[-150.0], [10.0]], "gamma": g})
    assert np.array_equal(enh(img, good).view(np.int32), want.view(np.int32))
    # the raw entry point: the bad image is NaN, the other one is computed, the status bit is set once
    p = dev.tensor(np.array([[5.0, 95.0, 0.4, 1.2], [10.0, 100.0, 0.7, 1.4]], np.float32))
    out = dev.diff_gated_f32(dev.tensor(img), p, True)
    assert dev.check_status(allow=_lib.STATUS_DIFF_RANK) == _lib.STATUS_DIFF_RANK
    assert dev.check_status() == 0
    out = out.cpu().numpy()
    assert np.isnan(out[1]).all() and np.array_equal(out[0].view(np.int32), want[0].view(np.int32))


def _predictor(torch, seed):
    """deep_learning_parameters.ParameterPredictor's layers (79 -> 256, three residual blocks, 128, four heads), eval mode."""
    nn = torch.nn
    torch.manual_seed(seed)

    class Block(nn.Module):
        def __init__(self, d):
            super().__init__()
            self.block = nn.Sequential(nn.Linear(d, d), nn.ReLU(), nn.Dropout(0.3), nn.Linear(d, d))

        def forward(self, x):
            return torch.relu(self.block(x) + x)

    class Predictor(nn.Module):
        def __init__(self):
            super().__init__()
            self.input_proj = nn.Sequential(nn.Linear(79, 256), nn.ReLU(), nn.Dropout(0.3))
            self.res_blocks = nn.ModuleList([Block(256) for _ in range(3)])
            self.output_proj = nn.Sequential(nn.Linear(256, 128), nn.ReLU())
            self.heads = nn.ModuleDict({k: nn.Linear(128, 1) for k in ("gamma", "L_low", "L_high", "use_gamma")})

        def forward(self, x):
            x = self.input_proj(x)
            for b in self.res_blocks:
                x = b(x)
            f = self.output_proj(x)
            return {"gamma": torch.sigmoid(self.heads["gamma"](f)) * 0.5 + 1.0,
                    "L_low": torch.sigmoid(self.heads["L_low"](f)) * 15 + 5,
                    "L_high": torch.sigmoid(self.heads["L_high"](f)) * 13 + 85,
                    "use_gamma": torch.sigmoid(self.heads["use_gamma"](f))}

    return Predictor().eval()


def test_one_end_to_end_training_step(dev):
    """features -> predictor -> module -> 0.5 L1 + 0.5 MSE -> backward (EndToEndTrainer.train_epoch, :265-290): the
    predictor's weight gradients match the same step through the restatement."""
    import torch

    import underwater_image_enhancement_amd as uw

    rng = np.random.default_rng(21)
    frames = rng.integers(0, 256, (4, 256, 256, 3), dtype=np.uint8)
    ref = dev.tensor(rng.random((4, 3, 256, 256), dtype=np.float32))
    feats = torch.as_tensor(uw.feature_extractor_rows(frames)).float().to(dev.torch_device)
    assert feats.shape == (4, 79)
    feats = (feats - feats.mean(0)) / (feats.std(0) + 1e-6)
    images = dev.tensor(np.ascontiguousarray(frames.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0))
    model = _predictor(torch, 1234).to(dev.torch_device)
    grads = []
    for module in (uw.GatedDifferentiableEnhancement(), None):
        model.zero_grad()
        params = model(feats)
        if module is None:
            out = R.gated(images, params["L_low"], params["L_high"], params["use_gamma"], params["gamma"])
        else:
            out = module(images, params)
        loss = 0.5 * torch.nn.functional.l1_loss(out, ref) + 0.5 * torch.nn.functional.mse_loss(out, ref)
        loss.backward()
        grads.append({k: None if v.grad is None else v.grad.detach().double().cpu().numpy() for k, v in model.named_parameters()})
    for k, want in grads[1].items():
        # the L_low / L_high heads get no gradient through either module (read with .item())
        assert (want is None) == (grads[0][k] is None) == k.startswith(("heads.L_low", "heads.L_high")), k
        if want is None:
            continue
        err = np.abs(grads[0][k] - want).max()
        assert err <= 1e-4 * np.abs(want).max(), f"{k}: off by {err:.3g} of max {np.abs(want).max():.3g}"


def test_a_training_loop_recovers_use_gamma_and_gamma(dev):
    import torch

    import underwater_image_enhancement_amd as uw

    rng = np.random.default_rng(7)
    B = 4
    x = dev.tensor(seeded((B, 3, 48, 64), rng))
    L = {"L_low": torch.full((B, 1), 5.0, device=dev.torch_device), "L_high": torch.full((B, 1), 95.0, device=dev.torch_device)}
    u_t = torch.tensor([[0.3], [0.6], [0.8], [0.45]], device=dev.torch_device)
    g_t = torch.tensor([[0.7], [1.4], [2.0], [1.2]], device=dev.torch_device)
    enh = uw.GatedDifferentiableEnhancement()
    with torch.no_grad():
        target = enh(x, {**L, "use_gamma": u_t, "gamma": g_t})
    u = torch.full((B, 1), 0.5, device=dev.torch_device, requires_grad=True)
    g = torch.full((B, 1), 1.0, device=dev.torch_device, requires_grad=True)
    opt = torch.optim.Adam([u, g], lr=0.05)
    first = None
    for _ in range(800):
        opt.zero_grad()
        loss = ((enh(x, {**L, "use_gamma": u, "gamma": g}) - target) ** 2).mean()
        loss.backward()
        opt.step()
        first = loss.item() if first is None else first
    last = ((enh(x, {**L, "use_gamma": u, "gamma": g}) - target) ** 2).mean().item()
    print(f"training loop: loss {first:.3g} -> {last:.3g}, |use_gamma error| {(u - u_t).abs().max().item():.2e}, "
          f"|gamma error| {(g - g_t).abs().max().item():.2e}")
    assert last * 1000 <= first
    assert (u - u_t).abs().max().item() < 0.02 and (g - g_t).abs().max().item() < 0.02
