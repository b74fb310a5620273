"""uw.resize_frames / image_tensor / vgg_input / training_batch on the device (uwie_resize_rgb_u8, k_resize.hip) against the
NumPy restatement tests/resize_ref.py (bit for bit) and the real reference datasets' items (tests/golden/train_batches.npz)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import resize_ref as R
from test_gpu_feature_extractor import assert_row

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_batches.npz")


@pytest.fixture(scope="module")
def uw():
    import underwater_image_enhancement_amd as uw

    return uw


@pytest.fixture(scope="module")
def dev(uw):
    return uw.get_device(0)


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        out = {k: z[k] for k in z.files}
    out["frame_hd_1080x1920"] = R.synth_frame(1080, 1920, 77)
    return out


GRID = [((480, 640), (224, 224)), ((300, 400), (256, 256)), ((200, 300), (128, 128)), ((37, 53), (100, 75)),
        ((75, 100), (100, 75)), ((20, 30), (224, 224)), ((9, 7), (64, 48)), ((448, 448), (224, 224)), ((256, 512), (256, 128)),
        ((53, 37), (37, 53)), ((1, 1), (5, 3)), ((1, 40), (13, 6)), ((40, 1), (6, 13)), ((600, 300), (225, 225)),
        ((123, 457), (1500, 1)), ((64, 64), (4096, 2))]


@pytest.mark.parametrize("src,dsize", GRID)
def test_u8_equals_the_restatement(uw, src, dsize):
    f = R.synth_frame(*src, seed=src[0] * 7 + src[1])
    frames = np.stack([f, 255 - f])
    got = uw.resize_frames(frames, dsize)
    assert got.shape == (2, dsize[1], dsize[0], 3) and got.dtype == np.uint8
    for i in range(2):
        assert np.array_equal(got[i], R.resize(frames[i], dsize)), (src, dsize, i)


@pytest.mark.parametrize("src,dsize,B", [((2160, 3840), (224, 224), 16), ((1080, 1920), (256, 256), 16)])
def test_large_batches_equal_the_restatement(uw, dev, src, dsize, B):
    base = R.synth_frame(*src, seed=5)
    frames = torch.stack([torch.from_numpy(np.roll(base, 17 * i, axis=1)) for i in range(B)]).to(dev.torch_device)
    got = uw.resize_frames(frames, dsize).cpu().numpy()
    for i in (0, 5, B - 1):
        assert np.array_equal(got[i], R.resize(np.roll(base, 17 * i, axis=1), dsize)), i


def test_ragged_list_equals_per_frame_calls(uw, dev):
    sizes = [(37, 53), (256, 256), (1080, 1920), (20, 30), (512, 512), (1, 7)]
    frames = [R.synth_frame(h, w, seed=i) for i, (h, w) in enumerate(sizes)]
    flips = [0, 1, 2, 3, 1, 0]
    got = uw.resize_frames(frames, (256, 256), flips=flips)
    for i, f in enumerate(frames):
        want = R.flip(R.resize(f, (256, 256)), flips[i])
        assert np.array_equal(got[i], want), sizes[i]
        assert np.array_equal(uw.resize_frames(f, (256, 256), flips=[flips[i]]), want)
    dev_frames = [torch.from_numpy(f).to(dev.torch_device) for f in frames]
    assert np.array_equal(uw.resize_frames(dev_frames, (256, 256), flips=flips).cpu().numpy(), got)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_float_planes_and_normalised_planes_bitwise(uw, flags):
    frames = [R.synth_frame(90, 160, 3), R.synth_frame(151, 67, 4)]
    want = np.stack([R.to_chw_f32(R.flip(R.resize(f, (100, 75)), flags)) for f in frames])
    got = uw.image_tensor(frames, (100, 75), flips=[flags, flags]).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(got, want)
    got = uw.image_tensor(frames, (100, 75), normalize="imagenet", flips=[flags, flags]).cpu().numpy()
    assert np.array_equal(got, R.normalize(want))
    m, s = (0.5, 0.25, 0.125), (0.3, 0.7, 1.9)
    got = uw.image_tensor(frames, (100, 75), normalize=(m, s), flips=[flags, flags]).cpu().numpy()
    assert np.array_equal(got, R.normalize(want, m, s))


def test_full_resolution_tensor_and_vgg_input(uw, golden):
    for name in ("odd_37x53", "small_30x20"):
        got = uw.image_tensor(golden["frame_" + name]).cpu().numpy()
        assert np.array_equal(got, golden[f"tensor/{name}"]), name
    for name in ("odd_37x53", "hd_1080x1920", "area_128x128"):
        size = int(golden[f"vgg/{name}/size"])
        got = uw.vgg_input(golden["frame_" + name], size=size).cpu().numpy()
        assert np.array_equal(got, golden[f"vgg/{name}"]), name


@pytest.mark.parametrize("group", ["dlp64", "dlp256", "vgg40", "vgg112", "vgg40_plain"])
def test_training_batch_equals_the_reference_items(uw, golden, group):
    names = [str(n) for n in golden[f"{group}/names"]]
    size, seed = int(golden[f"{group}/size"]), int(golden[f"{group}/seed"])
    images = [golden["frame_" + n] for n in names]
    refs = [golden.get("ref_" + n) for n in names]
    mode = "extractor" if group.startswith("dlp") else ("basic" if group != "vgg40_plain" else None)
    if seed >= 0:
        np.random.seed(seed)
    batch = uw.training_batch(images, refs, size=size, features=mode, augment=seed >= 0)
    img = golden[f"{group}/image"]
    assert np.array_equal(batch["image"].cpu().numpy(), R.to_chw_f32(img))
    ref = batch["reference"].cpu().numpy()
    want_ref, ri = [], 0
    for i, n in enumerate(names):
        if "ref_" + n in golden:
            want_ref.append(golden[f"{group}/reference"][ri])
            ri += 1
        else:
            want_ref.append(img[i])
    assert np.array_equal(ref, R.to_chw_f32(np.stack(want_ref)))
    feats = batch["features"].cpu().numpy()
    assert feats.dtype == np.float32 and feats.shape == golden[f"{group}/features"].shape
    if mode == "extractor":  # FeatureExtractor's float statistics: DESIGN.md section 9's tolerances
        for i in range(len(names)):
            assert_row(feats[i], golden[f"{group}/features"][i], f"{group}/{names[i]}")
    else:
        assert np.array_equal(feats, golden[f"{group}/features"])


def test_explicit_flips_override_the_draws(uw, golden):
    images = [golden["frame_odd_37x53"], golden["frame_wide_90x160"]]
    np.random.seed(0)
    a = uw.training_batch(images, size=40, features="basic", augment=True, flips=[3, 0])
    assert np.random.rand() == np.random.RandomState(0).rand()  # no draw was taken
    b = uw.training_batch(images, size=40, features="basic", flips=[3, 0])
    for k in ("image", "reference", "features"):
        assert torch.equal(a[k], b[k]), k
    want = R.flip(R.resize(images[0], (40, 40)), 3)
    assert np.array_equal(a["image"][0].cpu().numpy(), R.to_chw_f32(want))


def test_deterministic_across_runs_and_batch_compositions(uw, dev):
    frames = [R.synth_frame(h, w, seed=h) for h, w in ((1080, 1920), (37, 53), (512, 256), (300, 300))]
    one = uw.image_tensor(frames, (224, 224), normalize="imagenet", flips=[1, 2, 3, 0])
    two = uw.image_tensor(frames, (224, 224), normalize="imagenet", flips=[1, 2, 3, 0])
    assert torch.equal(one, two)
    for i in range(4):
        alone = uw.image_tensor([frames[i]], (224, 224), normalize="imagenet", flips=[[1, 2, 3, 0][i]])
        assert torch.equal(alone[0], one[i])
    rev = uw.image_tensor(frames[::-1], (224, 224), normalize="imagenet", flips=[0, 3, 2, 1])
    assert torch.equal(rev.flip(0), one)


def test_null_outputs_are_skipped(uw, dev):
    f = torch.from_numpy(R.synth_frame(90, 160, 1)).to(dev.torch_device)[None].contiguous()
    u8, f32, nrm = dev.resize_rgb(f, 40, 50, want_u8=False, want_f32=True)
    assert u8 is None and nrm is None
    u8b, f32b, nrmb = dev.resize_rgb(f, 40, 50, want_u8=True, want_f32=False, norm=(R.IMAGENET_MEAN, R.IMAGENET_STD))
    assert f32b is None
    want = R.resize(R.synth_frame(90, 160, 1), (50, 40))
    assert np.array_equal(u8b[0].cpu().numpy(), want)
    assert np.array_equal(f32.cpu().numpy()[0], R.to_chw_f32(want))
    assert np.array_equal(nrmb.cpu().numpy()[0], R.normalize(R.to_chw_f32(want)))
    assert dev.check_status() == 0


def test_argument_errors_raise(uw, dev):
    lib = dev.lib
    f = torch.zeros((1, 8, 8, 3), dtype=torch.uint8, device=dev.torch_device)
    table, _ = dev.frame_table(f)
    out = torch.empty((1, 4, 4, 3), dtype=torch.uint8, device=dev.torch_device)
    P = ctypes.c_void_p

    def call(batch=1, oh=4, ow=4, u8=out, desc=table):
        return lib.uwie_resize_rgb_u8(dev._ctx, P(desc.data_ptr()) if desc is not None else None, batch, oh, ow, None,
                                      P(u8.data_ptr()) if u8 is not None else None, None, None, None, None, dev.stream())

    assert call() == 0
    for kw in ({"oh": 0}, {"ow": -3}, {"oh": uw._lib.RESIZE_MAX_SIDE + 1}, {"batch": 0}, {"u8": None}, {"desc": None}):
        assert call(**kw) == -1, kw
    with pytest.raises(ValueError):
        uw.resize_frames(np.zeros((8, 8, 3), np.uint8), (0, 4))
    with pytest.raises(ValueError):
        uw.resize_frames(np.zeros((8, 8, 3), np.uint8), (4, 4), flips=[4])
    with pytest.raises(ValueError):
        uw.image_tensor([np.zeros((8, 8, 3), np.uint8), np.zeros((9, 8, 3), np.uint8)])
    with pytest.raises(TypeError):
        uw.resize_frames(np.zeros((8, 8, 3), np.float32), (4, 4))
    with pytest.raises(ValueError):
        uw.training_batch([np.zeros((8, 8, 3), np.uint8)], features="vgg")
    assert dev.check_status() == 0


def test_a_bad_descriptor_sets_the_status_bit(uw, dev):
    table = np.zeros(1, [("data", "<u8"), ("H", "<i4"), ("W", "<i4")])
    table["H"], table["W"] = 8, 8  # NULL data pointer: the kernel reads nothing
    d = torch.from_numpy(table.view(np.uint8)).to(dev.torch_device)
    out = torch.empty((1, 4, 4, 3), dtype=torch.uint8, device=dev.torch_device)
    assert dev.lib.uwie_resize_rgb_u8(dev._ctx, ctypes.c_void_p(d.data_ptr()), 1, 4, 4, None, ctypes.c_void_p(out.data_ptr()),
                                      None, None, None, None, dev.stream()) == 0
    assert dev.check_status(allow=32) == 32
    assert dev.check_status() == 0


def test_one_end_to_end_training_step(uw, dev):
    import torch.nn as nn

    torch.manual_seed(0)
    images = [R.synth_frame(h, w, seed=h) for h, w in ((480, 640), (300, 400), (256, 256), (1080, 1920))]
    refs = [R.synth_frame(h, w, seed=h + 1) for h, w in ((480, 640), (300, 400), (256, 256))] + [None]
    batch = uw.training_batch(images, refs, size=256, features="extractor")
    net = nn.Sequential(nn.Linear(79, 32), nn.ReLU(), nn.Linear(32, 4)).to(dev.torch_device)
    feats = batch["features"]
    feats = (feats - feats.mean(0)) / (feats.std(0) + 1e-6)
    raw = net(feats)
    params = {"L_low": (1 + 29 * torch.sigmoid(raw[:, 0:1])).detach(), "L_high": (65 + 34 * torch.sigmoid(raw[:, 1:2])).detach(),
              "use_gamma": torch.sigmoid(raw[:, 2:3]), "gamma": 1.0 + 0.5 * torch.sigmoid(raw[:, 3:4])}
    out = uw.GatedDifferentiableEnhancement()(batch["image"], params)
    loss = 0.5 * (out - batch["reference"]).abs().mean() + 0.5 * ((out - batch["reference"]) ** 2).mean()
    loss.backward()
    grads = [p.grad for p in net.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads)
    assert any(g.abs().sum() > 0 for g in grads)
    assert dev.check_status() == 0
