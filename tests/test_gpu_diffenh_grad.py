"""DifferentiableEnhancement's backward on the device: loss.backward() through the module against the real module's
gradients (tests/golden/vgg_grads.npz) and, at larger sizes, against the torch-CPU restatement (tests/diffenh_grad_ref.py).
Tolerances: DESIGN.md section 8."""
import os

import numpy as np
import pytest

import diffenh_grad_ref as R

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vgg_grads.npz")


@pytest.fixture(scope="module")
def dev():
    import underwater_image_enhancement_amd as uw

    return uw.get_device(0)


def golden_cases():
    with np.load(GOLDEN, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    tags = sorted({k.split("/")[0] for k in d})
    return {t: {k.split("/", 1)[1]: v for k, v in d.items() if k.startswith(t + "/")} for t in tags}


def run_module(dev, img, par, grad_out, img_grad=True):
    """loss.backward() through uw.DifferentiableEnhancement on device tensors -> (out, grad_img, {key: grad}, leaves)."""
    import torch

    import underwater_image_enhancement_amd as uw

    x = torch.from_numpy(np.ascontiguousarray(img)).to(dev.torch_device).requires_grad_(img_grad)
    leaves = {k: torch.from_numpy(np.asarray(v, np.float32)).to(dev.torch_device).requires_grad_(True) for k, v in par.items()}
    out = uw.DifferentiableEnhancement()(x, leaves)
    assert out.grad_fn is not None
    loss = (out * torch.from_numpy(np.asarray(grad_out, np.float32)).to(dev.torch_device)).sum()
    loss.backward()
    grads = {f"grad_{k}": leaves[k].grad.cpu().numpy() for k in ("omega", "gamma") if k in leaves}
    return out.detach().cpu().numpy(), (x.grad.cpu().numpy() if img_grad else None), grads, leaves, x


def params_of(c):
    return {k: c[k] for k in ("L_low", "L_high", "omega", "gamma") if k in c}


def test_gradients_match_the_real_module(dev):
    worst = 0.0
    for tag, c in golden_cases().items():
        par = params_of(c)
        out, gi, grads, leaves, _ = run_module(dev, c["img"], par, c["grad_out"])
        assert leaves["L_low"].grad is None and leaves["L_high"].grad is None, tag
        want = {"grad_img": c["grad_img_stable"], **{k: c[k] for k in ("grad_omega", "grad_gamma") if k in c}}
        got = {"grad_img": gi, **grads}
        w = R.check_grads(c["img"], c["L_low"], c["L_high"], c["grad_out"], got, want, tag=tag)
        worst = max(worst, w)
        if "gamma" not in par:
            # without pow every pointwise term is torch's own operation sequence: equal away from the scattered elements
            n = c["img"].shape[2] * c["img"].shape[3]
            diff = gi != c["grad_img_stable"]
            for b in range(c["img"].shape[0]):
                for ch in range(3):
                    for k in {int(R.sorted_positions(c["L_low"], n)[b]), int(R.sorted_positions(c["L_high"], n)[b])}:
                        diff[b, ch].reshape(-1)[R.stable_sort_source(c["img"][b, ch], k)] = False
            assert not diff.any(), f"{tag}: {np.count_nonzero(diff)} gradient elements differ without gamma"
    print(f"worst grad_img error over the module's cases: {worst:.3f} of the bound")


def seeded(shape, rng, u8=False):
    if u8:
        return np.float32(rng.integers(0, 256, shape)) / np.float32(255.0)
    return rng.random(shape, dtype=np.float32)


@pytest.mark.parametrize("shape,u8,planar", [((2, 3, 211, 157), False, True), ((2, 3, 211, 157), False, False),
                                             ((1, 3, 480, 640), True, True), ((1, 3, 480, 640), True, False),
                                             ((4, 3, 224, 224), False, True)])
def test_larger_cases_match_the_restatement(dev, shape, u8, planar):
    import underwater_image_enhancement_amd as uw

    rng = np.random.default_rng(hash((shape, u8, planar)) % 2**32)
    B = shape[0]
    img = seeded(shape, rng, u8)
    if not planar:
        img = np.ascontiguousarray(img.transpose(0, 2, 3, 1))
    L_low = rng.uniform(1, 30, (B, 1)).astype(np.float32)
    L_high = rng.uniform(65, 99, (B, 1)).astype(np.float32)
    omega = rng.uniform(0.1, 0.9, (B, 1)).astype(np.float32)
    gamma = rng.uniform(0.5, 3.0, (B, 1)).astype(np.float32)
    grad_out = rng.standard_normal(img.shape).astype(np.float32)
    _, want_img, want_om, want_ga = R.grads(img, L_low, L_high, omega, gamma, grad_out, planar=planar)
    x = dev.tensor(img).requires_grad_(True)
    p = dev.tensor(np.concatenate([L_low, L_high, omega, gamma], axis=1)).requires_grad_(True)
    out = uw.DiffEnhanceFunction.apply(x, p, 3, planar, dev)
    out.backward(dev.tensor(grad_out))
    gp = p.grad.cpu().numpy()
    assert not gp[:, :2].any()
    got = {"grad_img": x.grad.cpu().numpy(), "grad_omega": gp[:, 2:3], "grad_gamma": gp[:, 3:4]}
    want = {"grad_img": want_img, "grad_omega": want_om, "grad_gamma": want_ga}
    w = R.check_grads(img, L_low, L_high, grad_out, got, want, planar=planar, tag=f"{shape} planar={planar}")
    print(f"{shape} u8={u8} planar={planar}: worst grad_img error {w:.3f} of the bound")


@pytest.mark.parametrize("planar", [True, False])
def test_forward_with_grad_is_the_inference_forward(dev, planar):
    import torch

    import underwater_image_enhancement_amd as uw

    rng = np.random.default_rng(5)
    img = rng.random((3, 3, 37, 53) if planar else (3, 37, 53, 3), dtype=np.float32)
    p = np.concatenate([rng.uniform(1, 30, (3, 1)), rng.uniform(65, 99, (3, 1)), rng.uniform(0.1, 0.9, (3, 1)),
                        rng.uniform(0.5, 3.0, (3, 1))], axis=1).astype(np.float32)
    for flags in range(4):
        want = dev.diff_enhance_f32(dev.tensor(img), dev.tensor(p), planar, bool(flags & 1), bool(flags & 2))
        got = uw.DiffEnhanceFunction.apply(dev.tensor(img).requires_grad_(True), dev.tensor(p), flags, planar, dev)
        assert got.grad_fn is not None
        assert torch.equal(got.detach().view(torch.int32), want.view(torch.int32)), f"flags {flags}"


def test_backward_is_deterministic(dev):
    c = golden_cases()["u8ties_2x3x24x31"]
    rng = np.random.default_rng(9)
    img = seeded((4, 3, 224, 224), rng, u8=True)
    par = {"L_low": np.full((4, 1), 3.0, np.float32), "L_high": np.full((4, 1), 97.0, np.float32),
           "omega": rng.uniform(0.1, 0.9, (4, 1)).astype(np.float32), "gamma": rng.uniform(0.5, 3.0, (4, 1)).astype(np.float32)}
    grad_out = rng.standard_normal(img.shape).astype(np.float32)
    runs = [run_module(dev, img, par, grad_out) for _ in range(2)] + [run_module(dev, c["img"], params_of(c), c["grad_out"])
                                                                      for _ in range(2)]
    for a, b in ((runs[0], runs[1]), (runs[2], runs[3])):
        assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
        for k in a[2]:
            assert np.array_equal(a[2][k].view(np.int32), b[2][k].view(np.int32)), k


def test_parameter_gradients_alone(dev, monkeypatch):
    rng = np.random.default_rng(11)
    img = seeded((3, 3, 96, 80), rng, u8=True)
    par = {"L_low": rng.uniform(1, 30, (3, 1)).astype(np.float32), "L_high": rng.uniform(65, 99, (3, 1)).astype(np.float32),
           "omega": rng.uniform(0.1, 0.9, (3, 1)).astype(np.float32), "gamma": rng.uniform(0.5, 3.0, (3, 1)).astype(np.float32)}
    grad_out = rng.standard_normal(img.shape).astype(np.float32)
    _, _, with_img, _, _ = run_module(dev, img, par, grad_out, img_grad=True)
    seen = []
    real = dev.diff_enhance_bwd_f32

    def spy(*args, **kw):
        res = real(*args, **kw)
        seen.append(res[0] is None)
        return res

    monkeypatch.setattr(dev, "diff_enhance_bwd_f32", spy)
    _, gi, alone, _, x = run_module(dev, img, par, grad_out, img_grad=False)
    assert seen == [True], "the backward entry should get a NULL grad_img"
    assert x.grad is None and gi is None
    for k in with_img:
        assert np.array_equal(alone[k].view(np.int32), with_img[k].view(np.int32)), k


def test_low_precision_parameters_get_gradients_in_their_dtype(dev):
    import torch

    import underwater_image_enhancement_amd as uw

    rng = np.random.default_rng(13)
    x = dev.tensor(seeded((2, 3, 32, 48), rng))
    for dt in (torch.float16, torch.bfloat16):
        om = torch.tensor([[0.4], [0.7]], dtype=dt, device=dev.torch_device, requires_grad=True)
        ga = torch.tensor([[0.8], [1.6]], dtype=dt, device=dev.torch_device, requires_grad=True)
        out = uw.DifferentiableEnhancement()(x, {"L_low": torch.tensor([[5.0], [9.0]]), "L_high": torch.tensor([[95.0], [90.0]]),
                                                 "omega": om, "gamma": ga})
        out.mean().backward()
        assert om.grad.dtype == dt and ga.grad.dtype == dt and om.grad.shape == (2, 1)
        assert torch.isfinite(om.grad.float()).all() and (om.grad.float() != 0).any()


def test_a_small_training_loop_recovers_omega_and_gamma(dev):
    import torch

    import underwater_image_enhancement_amd as uw

    rng = np.random.default_rng(7)
    B = 4
    x = dev.tensor(seeded((B, 3, 48, 64), rng))
    L = {"L_low": torch.full((B, 1), 5.0, device=dev.torch_device), "L_high": torch.full((B, 1), 95.0, device=dev.torch_device)}
    om_t = torch.tensor([[0.35], [0.5], [0.65], [0.8]], device=dev.torch_device)
    ga_t = torch.tensor([[0.7], [1.4], [1.1], [1.8]], device=dev.torch_device)
    enh = uw.DifferentiableEnhancement()
    with torch.no_grad():
        target = enh(x, {**L, "omega": om_t, "gamma": ga_t})
    om = torch.full((B, 1), 0.55, device=dev.torch_device, requires_grad=True)
    ga = torch.full((B, 1), 1.0, device=dev.torch_device, requires_grad=True)
    opt = torch.optim.Adam([om, ga], lr=0.02)
    first = None
    for _ in range(300):
        opt.zero_grad()
        loss = ((enh(x, {**L, "omega": om, "gamma": ga}) - target) ** 2).mean()
        loss.backward()
        opt.step()
        first = loss.item() if first is None else first
    last = ((enh(x, {**L, "omega": om, "gamma": ga}) - target) ** 2).mean().item()
    print(f"training loop: loss {first:.3g} -> {last:.3g}, |omega error| {(om - om_t).abs().max().item():.2e}, "
          f"|gamma error| {(ga - ga_t).abs().max().item():.2e}")
    assert last * 100 <= first
    assert (om - om_t).abs().max().item() < 0.02 and (ga - ga_t).abs().max().item() < 0.02


def _exact_params(B):
    """Values float16 holds exactly, so every form below denotes the same float32 numbers."""
    return {"L_low": np.full((B, 1), 5.0), "L_high": np.full((B, 1), 95.0), "omega": np.full((B, 1), 0.75),
            "gamma": np.full((B, 1), 1.25)}


@pytest.mark.parametrize("keys", [("omega", "gamma"), ("omega",), ("gamma",), ()])
def test_inference_parameter_forms_give_the_binding_bytes(dev, keys):
    """Python floats, NumPy float64, CPU float64 tensors and device float16 tensors all go through the one column builder:
    each gives exactly the bytes of the Device binding with hand-built float32 [B,4] columns."""
    import torch

    import underwater_image_enhancement_amd as uw

    B, H, W = 2, 5, 7  # 35 pixels: an odd plane, not a multiple of any tile
    x = dev.tensor(np.random.default_rng(21).random((B, 3, H, W), dtype=np.float32))
    full = _exact_params(B)
    base = {k: v for k, v in full.items() if k in ("L_low", "L_high") + keys}
    pt = dev.tensor(np.concatenate([full["L_low"], full["L_high"], full["omega"] if "omega" in keys else np.zeros((B, 1)),
                                    full["gamma"] if "gamma" in keys else np.ones((B, 1))], axis=1).astype(np.float32))
    want = dev.diff_enhance_f32(x, pt, True, "omega" in keys, "gamma" in keys)
    forms = {"floats": {k: float(v[0, 0]) for k, v in base.items()},
             "numpy float64": {k: v.astype(np.float64) for k, v in base.items()},
             "cpu float64 tensors": {k: torch.from_numpy(v.astype(np.float64)) for k, v in base.items()},
             "device float16 tensors": {k: torch.from_numpy(v).to(device=dev.torch_device, dtype=torch.float16)
                                        for k, v in base.items()}}
    enh = uw.DifferentiableEnhancement()
    for name, params in forms.items():
        with torch.no_grad():
            got = enh(x, params)
        assert got.dtype == torch.float32 and got.grad_fn is None, name
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"{name}, keys {keys}"


def test_a_float64_torch_image_is_a_value_error_with_and_without_grad(dev):
    import torch

    import underwater_image_enhancement_amd as uw

    B = 2
    x = torch.from_numpy(np.random.default_rng(22).random((B, 3, 5, 7))).to(dev.torch_device)
    params = {k: torch.from_numpy(v.astype(np.float32)).to(dev.torch_device) for k, v in _exact_params(B).items()}
    enh = uw.DifferentiableEnhancement()
    with torch.no_grad(), pytest.raises(ValueError, match="float32 image batch"):
        enh(x, params)
    for requires in (False, True):  # grad mode on: the inference branch, then the grad branch
        params["omega"].requires_grad_(requires)
        with pytest.raises(ValueError, match="float32 image batch"):
            enh(x, params)
