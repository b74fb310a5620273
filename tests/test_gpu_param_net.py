"""ImprovedVGGParameterNet and EnhancementPredictor on the device: the golden of the real module
(tests/golden/param_net.npz) and the float64 restatement (tests/param_net_ref.py), the pooled vector's quirk, 224² frames,
determinism, the predictor's dicts and images, enhance_batch against single calls, and ImprovedTrainer.validate's step."""
import os

import numpy as np
import pytest

import param_net_ref as PN

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "param_net.npz")
PRED_SIZE = 48  # tests/gen_golden_param_net.py's EnhancementPredictor input_size


def golden():
    with np.load(GOLDEN, allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    tags = sorted({k.split("/")[0] for k in d if "/" in k})
    return int(d["seed"]), {t: {k.split("/", 1)[1]: v for k, v in d.items() if k.startswith(t + "/")} for t in tags}


@pytest.fixture(scope="module")
def dev():
    import underwater_image_enhancement_amd as uw

    return uw.get_device(0)


@pytest.fixture(scope="module")
def nets():
    import underwater_image_enhancement_amd as uw

    seed, _ = golden()
    return {uf: uw.VGGParameterNet(PN.seeded_state(seed, uf), use_features=uf) for uf in (True, False)}


def run(dev, net, img, feats):
    out = net(dev.tensor(img), None if feats is None else dev.tensor(feats), return_pooled=True)
    params = np.concatenate([out[k].cpu().numpy() for k in PN.KEYS], axis=1).astype(np.float64)
    return out["pooled"].cpu().numpy().astype(np.float64), params


def params_within(got, want, tol, what):
    for i, k in enumerate(PN.KEYS):
        lo, hi = PN.RANGES[k]
        err = np.abs(got[:, i] - want[:, i]).max() / (hi - lo)
        print(f"{what} {k}: {err:.3g} of the range")
        assert err <= tol, (what, k, err)


def test_golden_cases_against_float64_and_the_reference(dev, nets):
    seed, cases = golden()
    for tag, c in cases.items():
        if tag.startswith("pred_"):
            continue
        uf = bool(c["use_features"])
        pooled, params = run(dev, nets[uf], c["img"], c.get("features"))
        p64, q64 = PN.forward(PN.seeded_state(seed, uf), c["img"], c.get("features"), uf)
        err = np.abs(pooled - p64).max() / np.abs(p64).max()
        print(f"{tag}: pooled {err:.3g} of max |pooled|")
        assert err <= 1e-5, tag
        assert np.array_equal(pooled[:, 512:], pooled[:, :512]), tag
        params_within(params, q64, 1e-5, tag + " vs float64")
        params_within(params, c["params"].astype(np.float64), 2e-5, tag + " vs golden")


def test_224_frames_against_float64(dev, nets):
    seed, _ = golden()
    rng = np.random.default_rng(224)
    img = rng.standard_normal((4, 3, 224, 224)).astype(np.float32)
    feats = rng.random((4, 79), dtype=np.float32)
    _, params = run(dev, nets[True], img, feats)
    _, q64 = PN.forward(PN.seeded_state(seed), img, feats)
    params_within(params, q64, 1e-4, "4x3x224x224")


def test_two_runs_give_the_same_bits(dev, nets):
    rng = np.random.default_rng(5)
    img = rng.standard_normal((3, 3, 64, 72)).astype(np.float32)
    feats = rng.random((3, 79), dtype=np.float32)
    a = run(dev, nets[True], img, feats)
    b = run(dev, nets[True], img, feats)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_batch_rows_do_not_depend_on_the_batch(dev, nets):
    rng = np.random.default_rng(6)
    img = rng.standard_normal((3, 3, 24, 40)).astype(np.float32)
    feats = rng.random((3, 79), dtype=np.float32)
    _, whole = run(dev, nets[True], img, feats)
    for b in range(3):
        _, one = run(dev, nets[True], img[b:b + 1], feats[b:b + 1])
        assert np.array_equal(one, whole[b:b + 1])


@pytest.mark.parametrize("B", [8, 17, 33])
def test_linear_layers_staging_passes(dev, nets, B):
    """k_pn_linear stages 8192 // span batch rows per pass: 7 (fusion layer with features), 8 (without), 32 (the heads' first
    layers) and 16 (their last).  B = 8, 17 and 33 are one past a pass of 7, of 8 and 16, and of 32: on 8 x 8 frames every
    batch row equals its single call bit for bit, and the parameters stay within 1e-5 of their range of the float64 net."""
    seed, _ = golden()
    rng = np.random.default_rng(100 + B)
    img = rng.standard_normal((B, 3, 8, 8)).astype(np.float32)
    feats = rng.random((B, 79), dtype=np.float32)
    for uf in (True, False):
        f = feats if uf else None
        pooled, whole = run(dev, nets[uf], img, f)
        for b in range(B):
            p1, one = run(dev, nets[uf], img[b:b + 1], None if f is None else f[b:b + 1])
            assert np.array_equal(one, whole[b:b + 1]) and np.array_equal(p1, pooled[b:b + 1]), (uf, b)
        _, q64 = PN.forward(PN.seeded_state(seed, uf), img, f, uf)
        params_within(whole, q64, 1e-5, f"B={B} use_features={uf}")


def test_errors_before_any_launch(dev, nets):
    import torch

    with pytest.raises(RuntimeError):
        nets[True](dev.tensor(np.zeros((1, 3, 7, 16), np.float32)), dev.tensor(np.zeros((1, 79), np.float32)))
    with pytest.raises(RuntimeError):
        nets[True](dev.tensor(np.zeros((1, 3, 16, 16), np.float32)), None)
    out = nets[False](dev.tensor(np.zeros((1, 3, 16, 16), np.float32)), None)
    assert out["omega"].is_cuda and out["omega"].dtype == torch.float32


def test_autocast_and_cpu_tensors_take_the_torch_route(dev, nets):
    import torch

    rng = np.random.default_rng(8)
    img = rng.standard_normal((2, 3, 16, 16)).astype(np.float32)
    feats = rng.random((2, 79), dtype=np.float32)
    cpu = nets[True](torch.from_numpy(img), torch.from_numpy(feats))
    assert not cpu["omega"].is_cuda
    with torch.autocast("cuda", dtype=torch.float16):
        ac = nets[True](dev.tensor(img), dev.tensor(feats))
    assert ac["omega"].is_cuda


@pytest.fixture(scope="module")
def predictor():
    import underwater_image_enhancement_amd as uw

    seed, _ = golden()
    return uw.EnhancementPredictor(PN.seeded_state(seed), input_size=PRED_SIZE)


def test_predictor_on_the_golden_frames(dev, predictor):
    import underwater_image_enhancement_amd as uw

    seed, cases = golden()
    state = PN.seeded_state(seed)
    for tag, c in cases.items():
        if not tag.startswith("pred_"):
            continue
        frame = c["frame"]
        img = frame.astype(np.float32) / np.float32(255.0)
        want = dict(zip(c["keys"].tolist(), c["values"].tolist()))
        from_u8 = predictor.predict_parameters(frame)
        for x in (frame, img, frame / 255):  # uint8, float32 u8 / 255 and NumPy's float64 frame / 255
            got = predictor.predict_parameters(x)
            assert got == from_u8
            assert list(got) == list(want) and all(type(v) is float for v in got.values())
            g = np.array([[got[k] for k in PN.KEYS]])
            params_within(g, np.array([[want[k] for k in PN.KEYS]]), 2e-5, tag + " vs golden")
            assert got["guided_radius"] == 15.0 and got["use_gamma"] == 1.0
        enhanced = predictor.enhance_image(frame)
        assert np.array_equal(predictor.enhance_image(frame / 255), enhanced)
        assert np.array_equal(predictor.enhance_image(img), enhanced)
        # float64 restatement of the same chain: the device's VGG input and features, the network in float64
        x = uw.vgg_input(frame, PRED_SIZE).cpu().numpy()
        f = uw.extract_all_features(frame)[None]
        _, q64 = PN.forward(state, x, f)
        params_within(np.array([[got[k] for k in PN.KEYS]]), np.clip(q64, [0.1, 0.5, 1.0, 65.0], [0.9, 3.0, 30.0, 99.0]), 1e-5,
                      tag + " vs float64")
        # enhance_image with the golden's parameters: DifferentiableEnhancement's contract (pow within 1 float32 ulp)
        out = predictor.enhance_image(img, want)
        assert out.dtype == np.float32 and out.shape == frame.shape
        diff = np.abs(out.astype(np.float64) - c["enhanced"].astype(np.float64)).max()
        print(f"{tag}: enhance_image max |diff| {diff:.3g}")
        assert diff <= 2.0 ** -23
        assert np.array_equal(out, np.clip(uw.DifferentiableEnhancement().enhance_image(img, want), 0.0, 1.0))


def test_enhance_batch_equals_single_calls(dev, predictor):
    import underwater_image_enhancement_amd as uw

    rng = np.random.default_rng(11)
    frames = rng.integers(0, 256, (3, 40, 56, 3), dtype=np.uint8)
    out = predictor.enhance_batch(frames)
    assert out.is_cuda and tuple(out.shape) == (3, 40, 56, 3)
    host = out.cpu().numpy()
    params = predictor.predict_parameters(frames)
    for b in range(3):
        single = predictor.enhance_image(frames[b])
        assert np.array_equal(host[b], single), b
        one = predictor.predict_parameters(frames[b])
        assert all(params[k][b] == one[k] for k in one)
    assert np.array_equal(predictor.enhance_batch(dev.tensor(frames)).cpu().numpy(), host)
    with pytest.raises(uw.UnsupportedInputError):
        predictor.enhance_image(np.full((16, 16, 3), 0.5, np.float32))


def test_improved_trainer_validate_step(dev):
    """ImprovedTrainer.validate's step (vgg_16_UIE.py:563-586): net -> DifferentiableEnhancement -> CombinedLoss, the
    device route against the torch restatement of the net on the device, within N10's loss bounds."""
    import torch

    import perceptual_ref as PR
    import underwater_image_enhancement_amd as uw

    seed, _ = golden()
    net = uw.VGGParameterNet(PN.seeded_state(seed))
    crit = uw.CombinedLoss(weights=PR.seeded_weights(3))
    mod = uw.DifferentiableEnhancement()
    rng = np.random.default_rng(12)
    B, H, W = 2, 32, 40
    images = dev.tensor(rng.random((B, 3, H, W), dtype=np.float32))
    refs = dev.tensor(rng.random((B, 3, H, W), dtype=np.float32))
    feats = dev.tensor(rng.random((B, 79), dtype=np.float32))
    with torch.no_grad():
        loss, parts = crit(mod(images, net(images, feats)), refs)
        tm = net.torch_module(dev.torch_device)
        p_t = tm(images, feats)
        out_t = mod(images, p_t)
        vgg = crit.perceptual_loss.features(dev.torch_device)
        l1 = torch.nn.functional.l1_loss(out_t, refs).item()
        l2 = torch.nn.functional.mse_loss(out_t, refs).item()
        pe = torch.nn.functional.mse_loss(vgg(out_t), vgg(refs)).item()
    rel = lambda a, b: abs(a - b) / max(abs(b), 1e-30)  # noqa: E731
    print(parts, l1, l2, pe)
    assert rel(parts["l1"], l1) <= 1e-5 and rel(parts["l2"], l2) <= 1e-5
    assert rel(parts["perceptual"], pe) <= 1e-5
    assert rel(loss.item(), 0.3 * l1 + 0.5 * l2 + 0.2 * pe) <= 1e-5


def test_device_clamp_where_the_clip_bounds_act(dev):
    """Heads pushed into saturation: omega's sigmoid reaches 1 (0.6f + 0.3f = 0.90000004f, clipped to 0.9) and L_high's
    reaches 0 (60, clipped to 65).  The device clamp equals float32(np.clip(float(v), lo, hi)) of the raw outputs,
    predict_parameters gives the reference's float64 clip, and enhance_batch still equals single enhance_image calls."""
    import underwater_image_enhancement_amd as uw

    seed, _ = golden()
    state = PN.seeded_state(seed)
    state["param_heads.omega.3.bias"] = np.array([40.0], np.float32)
    state["param_heads.L_high.3.bias"] = np.array([-40.0], np.float32)
    pred = uw.EnhancementPredictor(state, input_size=PRED_SIZE)
    frames = np.random.default_rng(13).integers(0, 256, (2, 24, 32, 3), dtype=np.uint8)
    u8 = dev.tensor(frames)
    raw = pred._raw(dev, u8).cpu().numpy()
    assert np.all(raw[:, 0] == np.float32(0.6) + np.float32(0.3)) and np.all(raw[:, 3] == 60.0)
    lo = [uw.api.PREDICTOR_CLIP[k][0] for k in PN.KEYS]
    hi = [uw.api.PREDICTOR_CLIP[k][1] for k in PN.KEYS]
    want = np.clip(raw.astype(np.float64), lo, hi).astype(np.float32)
    got = pred._clamped(dev, u8).cpu().numpy()
    assert np.array_equal(got, want)
    assert np.all(got[:, 0] == np.float32(0.9)) and np.all(got[:, 3] == 65.0)
    params = pred.predict_parameters(frames)
    assert np.all(params["omega"] == 0.9) and np.all(params["L_high"] == 65.0)
    out = pred.enhance_batch(frames).cpu().numpy()
    for b in range(2):
        assert np.array_equal(out[b], pred.enhance_image(frames[b]))


def test_u8_to_f32_is_numpys_division(dev):
    rng = np.random.default_rng(14)
    for shape in ((2, 37, 53, 3), (1, 1, 1, 3), (5,)):
        x = rng.integers(0, 256, shape, dtype=np.uint8)
        got = dev.u8_to_f32(dev.tensor(x)).cpu().numpy()
        assert np.array_equal(got, x.astype(np.float32) / np.float32(255.0)), shape
    every = np.arange(256, dtype=np.uint8)
    assert np.array_equal(dev.u8_to_f32(dev.tensor(every)).cpu().numpy(), every / np.float32(255.0))
