"""PerceptualLoss and CombinedLoss on the device: the float32 route against the float64 restatement,
autocast's float16 route against the float16 restatement (tests/perceptual_ref.py), the max-pool tie rule bit for bit,
CombinedLoss against the unfused sequence, one ImprovedTrainer-shaped step, determinism and NaN inputs."""
import os

import numpy as np
import pytest

import perceptual_ref as PR

pytestmark = pytest.mark.gpu

SEED = 20261016
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "perceptual.npz")


@pytest.fixture(scope="module")
def dev():
    import underwater_image_enhancement_amd as uw

    return uw.get_device(0)


@pytest.fixture(scope="module")
def state():
    return PR.seeded_weights(SEED)


@pytest.fixture(scope="module")
def crit(state):
    import underwater_image_enhancement_amd as uw

    return uw.PerceptualLoss(state)


def rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)


def images(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.random(shape, dtype=np.float32), rng.random(shape, dtype=np.float32)


def device_loss(dev, crit, pred, target, g=1.0, autocast=False):
    import torch

    p = dev.tensor(pred).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16, enabled=autocast):
        loss = crit(p, dev.tensor(target))
    assert loss.dim() == 0 and loss.grad_fn is not None and loss.dtype == torch.float32
    (loss * g).backward()
    return float(loss.detach()), p.grad.double().cpu().numpy()


def grad_bound(got, want, tol):
    """||got - want||inf <= tol * ||want||inf per image."""
    for b in range(want.shape[0]):
        scale = np.abs(want[b]).max()
        err = np.abs(got[b] - want[b]).max()
        print(f"image {b}: |err|inf / |want|inf = {err / scale:.3g}")
        assert err <= tol * scale, f"image {b}: {err} > {tol} * {scale}"


def mean_rel(got, want):
    return np.abs(got - want).mean() / np.abs(want).mean()


@pytest.mark.parametrize("shape", [(2, 3, 37, 53), (1, 3, 4, 5), (3, 3, 16, 16)])
def test_float32_route_within_bounds_of_float64(dev, state, crit, shape):
    pred, target = images(shape, sum(shape))
    T = PR.tensors_of(state)
    l64, g64 = PR.loss_and_grad(pred, target, T, "f64")
    l32, g32 = PR.loss_and_grad(pred, target, T, "f32")
    loss, grad = device_loss(dev, crit, pred, target)
    # torch CPU float32 meets the same bounds: they are fair
    assert rel(l32, l64) <= 1e-5
    grad_bound(g32, g64, 1e-4)
    assert rel(loss, l64) <= 1e-5, (loss, float(l64))
    grad_bound(grad, g64, 1e-4)


def test_float32_route_at_224(dev, state, crit):
    """4 x 3 x 224 x 224 with random weights: a few ReLU masks and pool maxima flip between any two summation orders, each
    moving some gradient values by per cents, and torch CPU float32 itself misses 1e-4 * ||grad64||inf there (DESIGN.md
    section 14).  The loss meets 1e-5; the gradient is held to 5e-2 (infinity norm) and 1e-3 (mean)."""
    shape = (4, 3, 224, 224)
    pred, target = images(shape, sum(shape))
    T = PR.tensors_of(state)
    l64, g64 = PR.loss_and_grad(pred, target, T, "f64")
    l32, g32 = PR.loss_and_grad(pred, target, T, "f32")
    loss, grad = device_loss(dev, crit, pred, target)
    print("loss rel: device", rel(loss, l64), "torch cpu f32", rel(l32, l64))
    print("mean |diff| / mean |want|: device", mean_rel(grad, g64), "torch cpu f32", mean_rel(g32, g64))
    assert rel(loss, l64) <= 1e-5
    grad_bound(g32, g64, 5e-2)
    grad_bound(grad, g64, 5e-2)
    assert mean_rel(grad, g64) <= 1e-3


@pytest.mark.parametrize("shape,g", [((2, 3, 37, 53), 1.0), ((4, 3, 224, 224), 1.0), ((2, 3, 32, 48), 65536.0),
                                     ((4, 3, 224, 224), 65536.0)])
def test_float16_route_under_autocast(dev, state, crit, shape, g):
    """The loss within 2e-3 of the float16 restatement.  The gradient: float16 rounds the backward at every layer, exact
    pool ties are common in float16 and a one-ulp difference in a conv output moves a gradient to another element of its
    window, so the stated bounds (2e-2 infinity norm, 1e-3 mean) are not met by torch's own autocast route on the device
    either.  The device route is held to torch's own autocast route: its mean error against the restatement may not be
    larger (DESIGN.md section 14 has the numbers)."""
    import torch

    pred, target = images(shape, 7 + sum(shape))
    T = PR.tensors_of(state)
    want_l, want_g = PR.loss_and_grad(pred, target, T, "f16", g)
    loss, grad = device_loss(dev, crit, pred, target, g, autocast=True)
    vgg = crit.features(dev.torch_device)
    p = dev.tensor(pred).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.float16):
        tl = torch.nn.functional.mse_loss(vgg(p), vgg(dev.tensor(target)))
    (tl * g).backward()
    tg = p.grad.double().cpu().numpy()
    print("loss rel: device", rel(loss, want_l), "torch", rel(float(tl.detach()), want_l))
    print("mean |diff| / mean |want|: device", mean_rel(grad, want_g), "torch", mean_rel(tg, want_g))
    print("|diff|inf / |want|inf: device", np.abs(grad - want_g).max() / np.abs(want_g).max(),
          "torch", np.abs(tg - want_g).max() / np.abs(want_g).max())
    assert rel(loss, want_l) <= 2e-3, (loss, float(want_l))
    assert mean_rel(grad, want_g) <= mean_rel(tg, want_g)
    if g > 1.0 or shape[2] < 100:
        # where dL/dF stays in float16's normal range (GradScaler's factor, or small frames) the device route is also held
        # to a fixed 2e-2 mean: the contract itself moves by about 1 % between two float32 summation orders
        assert mean_rel(grad, want_g) <= 2e-2


def tie_state(mask):
    """Centre-tap-only weights of powers of two: every map is constant and positive, so every pool window ties, and every
    value is exact in float32.  ``mask``: odd output channels get a negative bias (ReLU zeroes them)."""
    state = {}
    for i, cin, cout in PR.CONVS:
        w = np.zeros((cout, cin, 3, 3), np.float32)
        w[:, :, 1, 1] = np.float32(2.0 ** -6) if cin > 3 else np.float32(0.25)
        b = np.full(cout, 2.0 ** -4, np.float32)
        if mask:
            b[1::2] = -8.0
        state[f"{i}.weight"], state[f"{i}.bias"] = w, b
    return state


@pytest.mark.parametrize("shape", [(1, 3, 10, 11), (2, 3, 8, 8)])
@pytest.mark.parametrize("mask", [False, True])
def test_pool_ties_go_to_the_top_left_element(dev, shape, mask):
    import underwater_image_enhancement_amd as uw

    st = tie_state(mask)
    pred = np.full(shape, 0.5, np.float32)
    target = np.full(shape, 0.25, np.float32)
    l32, want = PR.loss_and_grad(pred, target, PR.tensors_of(st), "f32")
    loss, grad = device_loss(dev, uw.PerceptualLoss(st), pred, target)
    assert loss == float(l32)
    assert np.array_equal(grad, want)
    H, W = shape[2], shape[3]
    keep = np.zeros((H, W), bool)
    keep[0:(H // 4) * 4:4, 0:(W // 4) * 4:4] = True
    assert np.all(grad[:, :, ~keep] == 0) and np.all(grad[:, :, keep] != 0)


def test_small_frames_raise_before_any_launch(dev, crit):
    import torch

    for shape in ((1, 3, 3, 8), (1, 3, 8, 2)):
        p = dev.tensor(np.zeros(shape, np.float32)).requires_grad_(True)
        with pytest.raises(RuntimeError):
            crit(p, dev.tensor(np.zeros(shape, np.float32)))
        with pytest.raises(RuntimeError):
            crit.features()(torch.zeros(shape))


def test_two_runs_give_the_same_bits_and_nan_propagates(dev, crit):
    pred, target = images((2, 3, 40, 36), 3)
    a = device_loss(dev, crit, pred, target)
    b = device_loss(dev, crit, pred, target)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    bad = pred.copy()
    bad[1, 2, 17, 9] = np.nan
    loss, grad = device_loss(dev, crit, bad, target)
    assert np.isnan(loss) and np.isnan(grad[1]).any()
    dev.check_status()
    c = device_loss(dev, crit, pred, target)
    assert c[0] == a[0] and np.array_equal(c[1], a[1])


def seeded_module_case(dev, shape, gated, seed):
    import torch

    rng = np.random.default_rng(seed)
    B = shape[0]
    img = rng.random(shape, dtype=np.float32)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(dev.torch_device)  # noqa: E731
    par = {"L_low": t(rng.uniform(5, 20, (B, 1))), "L_high": t(rng.uniform(85, 98, (B, 1)))}
    if gated:
        par.update(use_gamma=t(rng.uniform(0, 1, (B, 1))), gamma=t(rng.uniform(1.0, 1.5, (B, 1))))
    else:
        par.update(omega=t(rng.uniform(0.3, 0.95, (B, 1))), gamma=t(rng.uniform(0.5, 2.5, (B, 1))))
    return img, par, rng.random(shape, dtype=np.float32)


def fresh(dev, img, par):
    x = dev.tensor(img).requires_grad_(True)
    return x, {k: v.detach().clone().requires_grad_(k not in ("L_low", "L_high")) for k, v in par.items()}


def close(a, b, tol=1e-5):
    a, b = a.detach().double().cpu().numpy(), b.detach().double().cpu().numpy()
    assert np.abs(a - b).max() <= tol * max(np.abs(b).max(), 1e-30)


def test_combined_loss_on_tensors(dev, state):
    import torch

    import underwater_image_enhancement_amd as uw

    pred, target = images((2, 3, 48, 40), 11)
    cl = uw.CombinedLoss(weights=state)
    e = dev.tensor(pred).requires_grad_(True)
    total, parts = cl(e, dev.tensor(target))
    total.backward()
    e2 = dev.tensor(pred).requires_grad_(True)
    r = dev.tensor(target)
    l1 = torch.nn.functional.l1_loss(e2, r)
    l2 = torch.nn.functional.mse_loss(e2, r)
    p = cl.perceptual_loss(e2, r)
    (0.3 * l1 + 0.5 * l2 + 0.2 * p).backward()
    assert set(parts) == {"l1", "l2", "perceptual"}
    assert parts["perceptual"] == p.item()
    assert rel(parts["l1"], l1.item()) <= 1e-6 and rel(parts["l2"], l2.item()) <= 1e-6
    assert rel(total.item(), 0.3 * parts["l1"] + 0.5 * parts["l2"] + 0.2 * parts["perceptual"]) <= 1e-6
    close(e.grad, e2.grad)


@pytest.mark.parametrize("gated", [True, False])
def test_combined_through_matches_the_unfused_sequence(dev, state, gated):
    import torch

    import underwater_image_enhancement_amd as uw

    img, par, ref = seeded_module_case(dev, (2, 3, 64, 72), gated, 5 + gated)
    mod = uw.GatedDifferentiableEnhancement() if gated else uw.DifferentiableEnhancement()
    cl = uw.CombinedLoss(weights=state)
    r = dev.tensor(ref)
    x, leaves = fresh(dev, img, par)
    total, parts = cl.through(mod, x, leaves, r)
    total.backward()
    x2, leaves2 = fresh(dev, img, par)
    out = mod(x2, leaves2)
    l1 = torch.nn.functional.l1_loss(out, r)
    l2 = torch.nn.functional.mse_loss(out, r)
    p = cl.perceptual_loss(out, r)
    (0.3 * l1 + 0.5 * l2 + 0.2 * p).backward()
    assert parts["perceptual"] == p.item()  # the same output bytes through the same kernels
    assert rel(parts["l1"], l1.item()) <= 1e-6 and rel(parts["l2"], l2.item()) <= 1e-6
    close(x.grad, x2.grad)
    for k, v in leaves.items():
        if v.grad is not None:
            close(v.grad, leaves2[k].grad)


def test_improved_trainer_step(dev, state):
    """predictor -> module -> CombinedLoss.through -> backward: the predictor's gradients against the same step in torch
    (torch's vgg on the device for the perceptual term, the device module for the enhancement)."""
    import torch

    import underwater_image_enhancement_amd as uw

    torch.manual_seed(3)
    B, H, W = 2, 32, 40
    net = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.ReLU(), torch.nn.Linear(16, 2), torch.nn.Sigmoid()).to(dev.torch_device)
    rng = np.random.default_rng(9)
    feats = dev.tensor(rng.random((B, 8), dtype=np.float32))
    img = dev.tensor(rng.random((B, 3, H, W), dtype=np.float32))
    ref = dev.tensor(rng.random((B, 3, H, W), dtype=np.float32))
    mod = uw.DifferentiableEnhancement()
    cl = uw.CombinedLoss(weights=state)

    def params():
        o = net(feats)
        return {"L_low": torch.full((B, 1), 10.0, device=dev.torch_device), "L_high": torch.full((B, 1), 90.0, device=dev.torch_device),
                "omega": 0.3 + 0.6 * o[:, :1], "gamma": 0.5 + 1.5 * o[:, 1:]}

    net.zero_grad()
    total, _ = cl.through(mod, img, params(), ref)
    total.backward()
    got = [q.grad.clone() for q in net.parameters()]
    net.zero_grad()
    out = mod(img, params())
    vgg = cl.perceptual_loss.features(dev.torch_device)
    want = (0.3 * torch.nn.functional.l1_loss(out, ref) + 0.5 * torch.nn.functional.mse_loss(out, ref)
            + 0.2 * torch.nn.functional.mse_loss(vgg(out), vgg(ref)))
    want.backward()
    for g, q in zip(got, net.parameters()):
        close(g, q.grad, 1e-4)


def golden_cases():
    with np.load(GOLDEN, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    tags = sorted({k.split("/")[0] for k in d if "/" in k})
    return int(d["seed"]), {t: {k.split("/", 1)[1]: v for k, v in d.items() if k.startswith(t + "/")} for t in tags}


def test_golden_cases_of_the_reference_modules(dev):
    """tests/golden/perceptual.npz (the real vgg_16_UIE.PerceptualLoss / CombinedLoss, torch CPU float32): the float32 route
    within the float32 bounds of the float64 restatement and of the golden; CombinedLoss's parts and gradient."""
    import underwater_image_enhancement_amd as uw

    seed, cases = golden_cases()
    state = PR.seeded_weights(seed)
    crit = uw.PerceptualLoss(state)
    comb = uw.CombinedLoss(weights=state)
    T = PR.tensors_of(state)
    for tag, c in cases.items():
        loss, grad = device_loss(dev, crit, c["pred"], c["target"])
        e = dev.tensor(c["pred"]).requires_grad_(True)
        total, parts = comb(e, dev.tensor(c["target"]))
        total.backward()
        ge = e.grad.double().cpu().numpy()
        if "nan" in tag:
            assert np.isnan(loss) and np.isnan(grad).any() and np.isnan(parts["perceptual"]) and np.isnan(total.item())
            continue
        l64, g64 = PR.loss_and_grad(c["pred"], c["target"], T, "f64")
        assert rel(loss, l64) <= 1e-5 and rel(loss, c["perceptual"]) <= 1e-5, tag
        grad_bound(grad, g64, 1e-4)
        grad_bound(grad, c["grad_perceptual"].astype(np.float64), 2e-4)
        assert parts["perceptual"] == loss
        assert rel(parts["l1"], c["l1"]) <= 1e-6 and rel(parts["l2"], c["l2"]) <= 1e-6, tag
        assert rel(total.item(), c["total"]) <= 1e-5, tag
        grad_bound(ge, c["grad_enhanced"].astype(np.float64), 2e-4)


def test_pending_status_bits_survive_the_loss_calls(dev, state):
    """The perceptual calls neither read nor clear the device status word: a bit left pending by an earlier call (here the
    gated module's invalid sorted position, UWIE_STATUS_DIFF_RANK) is still there for its check afterwards."""
    from underwater_image_enhancement_amd import _lib

    import underwater_image_enhancement_amd as uw

    dev.check_status()
    rng = np.random.default_rng(12)
    img = dev.tensor(rng.random((1, 3, 16, 16), dtype=np.float32))
    pt = dev.tensor(np.array([[np.nan, 90.0, 0.5, 1.2]], np.float32))
    dev.ref_loss_f32(_lib.LOSS_GATED, img, pt, img.clone(), True)
    pred, target = images((2, 3, 16, 20), 13)
    e = dev.tensor(pred).requires_grad_(True)
    total, _ = uw.CombinedLoss(weights=state)(e, dev.tensor(target))
    total.backward()
    p = dev.tensor(pred).requires_grad_(True)
    uw.PerceptualLoss(state)(p, dev.tensor(target)).backward()
    assert dev.check_status(allow=_lib.STATUS_DIFF_RANK) == _lib.STATUS_DIFF_RANK


def test_device_argument_packs_both_precisions_at_construction(dev, state, crit):
    import underwater_image_enhancement_amd as uw

    eager = uw.PerceptualLoss(state, device=dev.index)
    assert len(eager._handles) == 2
    pred, target = images((1, 3, 20, 24), 21)
    a = device_loss(dev, eager, pred, target)
    b = device_loss(dev, crit, pred, target)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    eager.close()
