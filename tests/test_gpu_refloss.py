"""ReferenceLoss on the device: the stand-alone loss against torch CPU autograd, the loss fused into
the two enhancement modules' sweeps against the real modules (tests/golden/refloss.npz), against the unfused device step
and against the torch restatements (tests/dlp_grad_ref.py, tests/diffenh_grad_ref.py), and one EndToEndTrainer step."""
import os

import numpy as np
import pytest

import diffenh_grad_ref as RV
import dlp_grad_ref as RG

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refloss.npz")
GATED_KEYS = ("L_low", "L_high", "use_gamma", "gamma")


@pytest.fixture(scope="module")
def dev():
    import underwater_image_enhancement_amd as uw

    return uw.get_device(0)


def golden_cases():
    with np.load(GOLDEN, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    tags = sorted({k.split("/")[0] for k in d})
    return {t: {k.split("/", 1)[1]: v for k, v in d.items() if k.startswith(t + "/")} for t in tags}


def rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)


def bits(t):
    import torch

    return t.detach().contiguous().view(torch.int32).cpu().numpy()


# ------------------------------------------------------------------ identity map: the stand-alone loss
@pytest.mark.parametrize("shape", [(2, 3, 17, 19), (4, 3, 256, 256), (1, 3, 5, 7)])
@pytest.mark.parametrize("w1,w2,up", [(0.5, 0.5, 1.0), (0.3, 0.5, 1.0), (0.5, 0.5, 3.7), (1.3, 0.7, -2.1)])
def test_identity_gradient_is_torch_cpu_autograd_bit_for_bit(dev, shape, w1, w2, up):
    import torch

    import underwater_image_enhancement_amd as uw

    rng = np.random.default_rng(sum(shape) + int(10 * abs(up)))
    o = rng.random(shape, dtype=np.float32)
    r = rng.random(shape, dtype=np.float32)
    r.reshape(-1)[::5] = o.reshape(-1)[::5]  # sgn(0) = 0
    oc = torch.from_numpy(o.copy()).requires_grad_(True)
    l1 = torch.nn.functional.l1_loss(oc, torch.from_numpy(r))
    l2 = torch.nn.functional.mse_loss(oc, torch.from_numpy(r))
    (up * (w1 * l1 + w2 * l2)).backward()
    og = dev.tensor(o).requires_grad_(True)
    loss, parts = uw.ReferenceLoss(w1, w2)(og, dev.tensor(r))
    assert loss.grad_fn is not None and loss.dim() == 0
    (up * loss).backward()
    assert np.array_equal(bits(og.grad), oc.grad.numpy().view(np.int32))
    d = (o - r)
    s1, s2 = np.abs(d).astype(np.float64).sum() / d.size, (d * d).astype(np.float64).sum() / d.size
    assert rel(parts["l1"], s1) <= 1e-6 and rel(parts["l2"], s2) <= 1e-6
    assert rel(parts["l1"], l1.item()) <= 1e-5 and rel(parts["l2"], l2.item()) <= 1e-5
    assert rel(loss.item(), w1 * np.float32(parts["l1"]) + w2 * np.float32(parts["l2"])) <= 1e-6


def test_identity_takes_any_layout_and_the_upstream_output(dev):
    import torch

    import underwater_image_enhancement_amd as uw

    rng = np.random.default_rng(8)
    o = rng.random((5, 7, 3), dtype=np.float32)
    r = rng.random((5, 7, 3), dtype=np.float32)
    og = dev.tensor(o).requires_grad_(True)
    l1, l2 = uw.RefLossFunction.apply(og.view(1, 3, 1, -1), dev.tensor(r).view(1, 3, 1, -1), dev)
    (0.25 * l1).backward()
    oc = torch.from_numpy(o.copy()).requires_grad_(True)
    (0.25 * torch.nn.functional.l1_loss(oc, torch.from_numpy(r))).backward()
    assert np.array_equal(bits(og.grad), oc.grad.numpy().view(np.int32))
    loss, parts = uw.ReferenceLoss()(dev.tensor(o), dev.tensor(r))  # (5, 7, 3): not (B, 3, H, W)
    assert rel(parts["l1"], torch.nn.functional.l1_loss(torch.from_numpy(o), torch.from_numpy(r)).item()) <= 1e-5


# ------------------------------------------------------------------ the fused modules against the real ones
def module_and_params(uw, torch, dev, c):
    keys = GATED_KEYS if int(c["kind"]) == 0 else tuple(k for k in ("L_low", "L_high", "omega", "gamma") if k in c)
    mod = uw.GatedDifferentiableEnhancement() if int(c["kind"]) == 0 else uw.DifferentiableEnhancement()
    leaves = {k: torch.from_numpy(np.asarray(c[k], np.float32)).to(dev.torch_device).requires_grad_(True) for k in keys}
    return mod, leaves


def test_fused_step_matches_the_real_modules(dev):
    import torch

    import underwater_image_enhancement_amd as uw

    worst = 0.0
    for tag, c in golden_cases().items():
        mod, leaves = module_and_params(uw, torch, dev, c)
        x = dev.tensor(c["img"]).requires_grad_(True)
        w1, w2 = (float(v) for v in c["w"])
        loss, parts = uw.ReferenceLoss(w1, w2).through(mod, x, leaves, dev.tensor(c["ref"]))
        loss.backward()
        assert leaves["L_low"].grad is None and leaves["L_high"].grad is None, tag
        gated = int(c["kind"]) == 0
        pkeys = ("use_gamma", "gamma") if gated else tuple(k for k in ("omega", "gamma") if k in leaves)
        if "nan" in tag:
            assert np.isnan(parts["l1"]) and np.isnan(parts["l2"]) and np.isnan(loss.item()), tag
            for k in pkeys:
                got = leaves[k].grad.cpu().numpy()
                assert np.array_equal(np.isnan(got), np.isnan(c["grad_" + k])), (tag, k)
            continue
        assert rel(parts["l1"], c["l1"]) <= 1e-5 and rel(parts["l2"], c["l2"]) <= 1e-5, (tag, parts, c["l1"], c["l2"])
        assert rel(loss.item(), c["total"]) <= 2e-5, tag
        got = {"grad_img": x.grad.cpu().numpy(), **{"grad_" + k: leaves[k].grad.cpu().numpy() for k in pkeys}}
        want = {"grad_img": c["grad_img_stable"], **{"grad_" + k: c["grad_" + k] for k in pkeys}}
        R = RG if gated else RV
        worst = max(worst, R.check_grads(c["img"], c["L_low"], c["L_high"], c["grad_out"], got, want, tag=tag))
    print(f"worst grad_img error over the fixture's cases: {worst:.3f} of the bound")


def unfused(uw, dev, mod, x, leaves, ref, w1, w2, extra=None):
    """module -> the stand-alone ReferenceLoss on its output -> backward: (parts, grad_img, {key: grad})."""
    out = mod(x, leaves)
    loss, parts = uw.ReferenceLoss(w1, w2)(out, ref)
    if extra is not None:
        loss = loss + extra(out)
    loss.backward()
    return parts, x.grad, {k: v.grad for k, v in leaves.items() if v.grad is not None}


def fresh(dev, img, par):
    x = dev.tensor(img).requires_grad_(True)
    return x, {k: v.detach().clone().requires_grad_(k not in ("L_low", "L_high")) for k, v in par.items()}


def seeded_case(torch, dev, shape, gated, seed):
    rng = np.random.default_rng(seed)
    B = shape[0]
    img = np.float32(rng.integers(0, 256, shape)) / np.float32(255.0) if seed % 2 else rng.random(shape, dtype=np.float32)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev.torch_device)  # noqa: E731
    par = {"L_low": t(rng.uniform(5, 20, (B, 1))), "L_high": t(rng.uniform(85, 98, (B, 1)))}
    if gated:
        par.update(use_gamma=t(rng.uniform(0, 1, (B, 1))), gamma=t(rng.uniform(1.0, 1.5, (B, 1))))
    else:
        par.update(omega=t(rng.uniform(0.3, 0.95, (B, 1))), gamma=t(rng.uniform(0.5, 2.5, (B, 1))))
    ref = rng.random(shape, dtype=np.float32)
    return img, par, ref


@pytest.mark.parametrize("shape", [(4, 3, 256, 256), (2, 3, 1080, 1920)])
@pytest.mark.parametrize("gated", [True, False])
def test_fused_matches_the_unfused_step_and_the_restatement(dev, shape, gated):
    import torch

    import underwater_image_enhancement_amd as uw

    img, par, ref = seeded_case(torch, dev, shape, gated, sum(shape) + gated)
    mod = uw.GatedDifferentiableEnhancement() if gated else uw.DifferentiableEnhancement()
    r = dev.tensor(ref)
    x, leaves = fresh(dev, img, par)
    loss, parts = uw.ReferenceLoss(0.5, 0.5).through(mod, x, leaves, r)
    loss.backward()
    dev.check_status()
    x2, leaves2 = fresh(dev, img, par)
    parts2, gi2, gp2 = unfused(uw, dev, mod, x2, leaves2, r, 0.5, 0.5)
    # the same forward values in the same per-block order, the same dL/d(out): the fused step is the module step followed
    # by the stand-alone loss, bit for bit
    assert parts == parts2
    assert np.array_equal(bits(x.grad), bits(gi2)), "grad_img: fused != unfused"
    for k, g in gp2.items():
        assert np.array_equal(bits(leaves[k].grad), bits(g)), k
    # the torch restatement on the CPU, with dL/d(out) from its own output
    cpu = {k: v.cpu().numpy() for k, v in par.items()}
    if gated:
        xo = torch.from_numpy(img)
        o = RG.gated(xo, *(torch.from_numpy(cpu[k]) for k in GATED_KEYS)).requires_grad_(True)
    else:
        o = RV.diff_enhance(torch.from_numpy(img), torch.from_numpy(cpu["L_low"]), torch.from_numpy(cpu["L_high"]),
                            torch.from_numpy(cpu["omega"]), torch.from_numpy(cpu["gamma"])).requires_grad_(True)
    o = o.detach().requires_grad_(True)
    rc = torch.from_numpy(ref)
    (0.5 * torch.nn.functional.l1_loss(o, rc) + 0.5 * torch.nn.functional.mse_loss(o, rc)).backward()
    go = o.grad.numpy()
    assert rel(parts["l1"], torch.nn.functional.l1_loss(o, rc).item()) <= 1e-5
    if gated:
        _, wi, wu, wg = RG.grads(img, cpu["L_low"], cpu["L_high"], cpu["use_gamma"], cpu["gamma"], go)
        want = {"grad_img": wi, "grad_use_gamma": wu, "grad_gamma": wg}
        got = {"grad_img": x.grad.cpu().numpy(), "grad_use_gamma": leaves["use_gamma"].grad.cpu().numpy(),
               "grad_gamma": leaves["gamma"].grad.cpu().numpy()}
    else:
        _, wi, wo, wg = RV.grads(img, cpu["L_low"], cpu["L_high"], cpu["omega"], cpu["gamma"], go)
        want = {"grad_img": wi, "grad_omega": wo, "grad_gamma": wg}
        got = {"grad_img": x.grad.cpu().numpy(), "grad_omega": leaves["omega"].grad.cpu().numpy(),
               "grad_gamma": leaves["gamma"].grad.cpu().numpy()}
    R = RG if gated else RV
    w = R.check_grads(img, cpu["L_low"], cpu["L_high"], go, got, want, tag=f"{shape} gated={gated}")
    print(f"{shape} gated={gated}: worst grad_img error {w:.3f} of the bound")


@pytest.mark.parametrize("gated", [True, False])
def test_with_loss_keeps_the_inference_output_and_takes_an_extra_term(dev, gated):
    import torch

    import underwater_image_enhancement_amd as uw

    img, par, ref = seeded_case(torch, dev, (3, 3, 61, 47), gated, 11 + gated)
    mod = uw.GatedDifferentiableEnhancement() if gated else uw.DifferentiableEnhancement()
    r = dev.tensor(ref)
    with torch.no_grad():
        want_out = mod(dev.tensor(img), par)
    wmap = dev.tensor(np.random.default_rng(2).standard_normal(img.shape).astype(np.float32))
    perceptual = lambda out: 0.2 * (out * wmap).mean()  # noqa: E731  stands in for CombinedLoss's VGG term
    x, leaves = fresh(dev, img, par)
    out, l1, l2 = mod.with_loss(x, leaves, r)
    assert np.array_equal(bits(out), bits(want_out))
    assert out.grad_fn is not None and l1.grad_fn is not None and l1.dim() == 0
    (0.3 * l1 + 0.5 * l2 + perceptual(out)).backward()
    x2, leaves2 = fresh(dev, img, par)
    parts2, gi2, gp2 = unfused(uw, dev, mod, x2, leaves2, r, 0.3, 0.5, extra=perceptual)
    assert l1.item() == parts2["l1"] and l2.item() == parts2["l2"]
    # dL/d(out) is a three-term sum whose order is autograd's: 1 ulp of the largest term, then the module's backward
    gi, gw = x.grad.cpu().numpy().astype(np.float64), gi2.cpu().numpy().astype(np.float64)
    assert np.abs(gi - gw).max() <= 1e-5 * np.abs(gw).max()
    for k, g in gp2.items():
        a, b = leaves[k].grad.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
        assert (np.abs(a - b) <= 1e-5 * np.maximum(np.abs(b), 1e-3)).all(), (k, a, b)
    # without a caller's term on out the output still carries no extra gradient work
    x3, leaves3 = fresh(dev, img, par)
    out3, m1, m2 = mod.with_loss(x3, leaves3, r)
    (0.5 * m1 + 0.5 * m2).backward()
    x4, leaves4 = fresh(dev, img, par)
    loss4, _ = uw.ReferenceLoss().through(mod, x4, leaves4, r)
    loss4.backward()
    assert np.array_equal(bits(x3.grad), bits(x4.grad))


def test_one_end_to_end_training_step_through_the_fused_loss(dev):
    """EndToEndTrainer.train_epoch (:265-290) with crit.through: the predictor's weight gradients match the unfused step."""
    import torch

    import underwater_image_enhancement_amd as uw
    from test_gpu_dlp_grad import _predictor

    rng = np.random.default_rng(21)
    frames = rng.integers(0, 256, (4, 256, 256, 3), dtype=np.uint8)
    ref = dev.tensor(rng.random((4, 3, 256, 256), dtype=np.float32))
    feats = torch.as_tensor(uw.feature_extractor_rows(frames)).float().to(dev.torch_device)
    feats = (feats - feats.mean(0)) / (feats.std(0) + 1e-6)
    images = dev.tensor(np.ascontiguousarray(frames.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0))
    model = _predictor(torch, 1234).to(dev.torch_device)
    crit = uw.ReferenceLoss(l1_weight=0.5, l2_weight=0.5)
    grads, parts_seen = [], []
    for fused in (True, False):
        model.zero_grad()
        params = model(feats)
        if fused:
            loss, parts = crit.through(uw.GatedDifferentiableEnhancement(), images, params, ref)
        else:
            out = R_gated(params, images)
            loss, parts = crit(out, ref)
        parts_seen.append(parts)
        loss.backward()
        grads.append({k: None if v.grad is None else v.grad.detach().double().cpu().numpy() for k, v in model.named_parameters()})
    for key in ("l1", "l2"):
        assert rel(parts_seen[0][key], parts_seen[1][key]) <= 1e-5
    for k, want in grads[1].items():
        assert (want is None) == (grads[0][k] is None) == k.startswith(("heads.L_low", "heads.L_high")), k
        if want is None:
            continue
        err = np.abs(grads[0][k] - want).max()
        assert err <= 1e-4 * np.abs(want).max(), f"{k}: off by {err:.3g} of max {np.abs(want).max():.3g}"


def R_gated(params, images):
    return RG.gated(images, params["L_low"], params["L_high"], params["use_gamma"], params["gamma"])


def test_two_runs_give_the_same_bits(dev):
    import torch

    import underwater_image_enhancement_amd as uw

    img, par, ref = seeded_case(torch, dev, (2, 3, 300, 257), True, 5)
    runs = []
    for _ in range(2):
        x, leaves = fresh(dev, img, par)
        loss, parts = uw.ReferenceLoss(0.3, 0.5).through(uw.GatedDifferentiableEnhancement(), x, leaves, dev.tensor(ref))
        loss.backward()
        runs.append((bits(loss), parts, bits(x.grad), bits(leaves["use_gamma"].grad), bits(leaves["gamma"].grad)))
    a, b = runs
    assert a[1] == b[1]
    for u, v in zip(a[:1] + a[2:], b[:1] + b[2:]):
        assert np.array_equal(u, v)


def test_unindexable_positions_raise_and_the_device_carries_on(dev):
    import torch

    import underwater_image_enhancement_amd as uw

    rng = np.random.default_rng(3)
    img = rng.random((2, 3, 8, 8), dtype=np.float32)
    ref = dev.tensor(rng.random((2, 3, 8, 8), dtype=np.float32))
    enh = uw.GatedDifferentiableEnhancement()
    crit = uw.ReferenceLoss()
    good = {"L_low": [[5.0], [10.0]], "L_high": [[95.0], [90.0]], "use_gamma": [[0.4], [0.7]], "gamma": [[1.2], [1.4]]}
    want, want_parts = crit.through(enh, img, good, ref)
    with pytest.raises(IndexError, match="index 64 is out of bounds"):
        crit.through(enh, img, {**good, "L_high": [[95.0], [100.0]]}, ref)
    with pytest.raises(ValueError):
        crit.through(enh, img, {**good, "L_low": [[np.nan], [10.0]]}, ref)
    with pytest.raises(OverflowError):
        enh.with_loss(img, {**good, "L_low": [[5.0], [np.inf]]}, ref)
    # the module's error comes before the loss's own shape error
    with pytest.raises(IndexError):
        crit.through(enh, img, {**good, "L_low": [[-150.0], [10.0]]}, ref[:1])
    with pytest.raises(ValueError, match="does not match"):
        crit.through(enh, img, good, ref[:1])
    with pytest.raises(ValueError, match="float32"):
        crit.through(enh, img, good, ref.double())
    with pytest.raises(ValueError, match="float32"):
        crit.through(enh, dev.tensor(img).double(), good, ref)
    again, parts = crit.through(enh, img, good, ref)
    assert parts == want_parts and torch.equal(again, want)
    assert dev.check_status() == 0
