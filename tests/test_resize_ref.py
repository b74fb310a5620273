"""Known-answer tests of tests/resize_ref.py, the NumPy restatement of cv2.resize's fixed-point INTER_LINEAR on u8 frames
and of the trainer's per-frame preparation, and of tests/golden/train_batches.npz against it."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import features79_ref as F79
import resize_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "train_batches.npz")


def rnd(H, W, C=3, seed=0):
    shape = (H, W, C) if C else (H, W)
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


@pytest.mark.parametrize("H,W", [(200, 300), (256, 256), (128, 128), (129, 131), (300, 129), (1080, 1920), (150, 1000)])
def test_gray_downscale_equals_resize128(H, W):
    g = rnd(H, W, 0, seed=H + W)
    assert np.array_equal(R.resize(g, (128, 128)), F79.resize128(g))


def test_rgb_channels_are_the_gray_resize_of_each_channel_where_there_is_no_tail():
    f = rnd(200, 300, seed=1)
    out = R.resize(f, (128, 128))  # 384 bytes a row: no tail
    for c in range(3):
        assert np.array_equal(out[:, :, c], F79.resize128(np.ascontiguousarray(f[:, :, c])))


def test_upscale_rows_keep_their_fraction():
    """On an upscale resize128 clamps the row fraction at the borders; OpenCV's rows only clip the indices."""
    g = np.full((8, 8), 0, np.uint8)
    g[0] = 200
    a, b = R.resize(g, (128, 128)), F79.resize128(g)
    assert np.array_equal(a[8:-8], b[8:-8])  # the interior agrees


@pytest.mark.parametrize("H,W,ow,oh", [(7, 9, 5, 3), (10, 33, 100, 3), (1, 1, 4, 3), (1, 5, 3, 2), (6, 1, 2, 9), (8, 8, 4, 4),
                                       (8, 8, 8, 8), (5, 7, 11, 13), (40, 30, 17, 23)])
def test_scalar_evaluation_equals_vectorised(H, W, ow, oh):
    f = rnd(H, W, seed=H * 31 + W)
    assert np.array_equal(R.resize(f, (ow, oh)), R.resize_scalar(f, (ow, oh)))


@pytest.mark.parametrize("dsize", [(224, 224), (100, 75), (7, 300), (1, 1), (500, 3)])
def test_constant_frames_stay_constant(dsize):
    f = np.empty((37, 53, 3), np.uint8)
    f[:] = (0, 137, 255)
    out = R.resize(f, dsize)
    assert out.shape == (dsize[1], dsize[0], 3)
    assert np.all(out == np.array([0, 137, 255], np.uint8))


def test_equal_size_is_a_copy():
    f = rnd(37, 53, seed=3)
    out = R.resize(f, (53, 37))
    assert np.array_equal(out, f) and out is not f


def test_exact_2x_is_area_average():
    f = np.zeros((4, 6, 3), np.uint8)
    f[0:2, 0:2, 0] = [[1, 2], [2, 2]]  # sum 7 -> (7 + 2) >> 2 = 2
    f[0:2, 2:4, 0] = [[1, 1], [1, 2]]  # sum 5 -> 1
    f[2:4, 4:6] = 255
    out = R.resize(f, (3, 2))
    assert out[0, 0, 0] == 2 and out[0, 1, 0] == 1 and out[1, 2, 0] == 255 and out[1, 0, 0] == 0
    # 3x stays linear: taps at source 1, 4 (scale 3: fx = 3 d + 1, fraction 0)
    g = rnd(6, 9, seed=4)
    assert np.array_equal(R.resize(g, (3, 2)), g[1::3, 1::3])


def test_one_pixel_sources():
    px = np.array([[[10, 20, 30]]], np.uint8)
    assert np.all(R.resize(px, (5, 4)) == px)
    row = rnd(1, 9, seed=5)
    out = R.resize(row, (4, 3))
    # every output row reads the same source row twice; the split coefficients' rounding moves a byte by at most 1
    assert np.abs(out.astype(int) - R.resize(row, (4, 1)).astype(int)).max() <= 1
    col = rnd(9, 1, seed=6)
    out = R.resize(col, (5, 4))
    assert np.all(out == out[:, 0:1])


def test_upscale_and_non_square_shapes():
    f = rnd(10, 12, seed=7)
    for dsize in ((24, 20), (37, 5), (5, 37), (100, 75)):
        out = R.resize(f, dsize)
        assert out.shape == (dsize[1], dsize[0], 3)
        assert out.min() >= f.min() and out.max() <= f.max()


def test_tail_rule():
    assert R.vertical_tail_start(224 * 3) == 672 and R.vertical_tail_start(256 * 3) == 768 and R.vertical_tail_start(128) == 128
    assert R.vertical_tail_start(300) == 296 and R.vertical_tail_start(12) == 8 and R.vertical_tail_start(8) == 0
    assert R.vertical_tail_start(24) == 16 and R.vertical_tail_start(25) == 24


@pytest.mark.parametrize("H,W,ow,oh", [(1080, 1920, 256, 256), (300, 400, 224, 224), (50, 60, 100, 75), (33, 47, 20, 90)])
def test_within_one_of_float_bilinear(H, W, ow, oh):
    """An independent sanity check, not a contract: torch's float64 bilinear (align_corners=False, no antialias)."""
    f = R.synth_frame(H, W, 9)
    t = torch.from_numpy(f.astype(np.float64)).permute(2, 0, 1)[None]
    want = F.interpolate(t, size=(oh, ow), mode="bilinear", align_corners=False, antialias=False)[0].permute(1, 2, 0).numpy()
    got = R.resize(f, (ow, oh)).astype(np.float64)
    assert np.abs(got - np.rint(want)).max() <= 1


def test_normalize_equals_torch_bitwise():
    u8 = rnd(17, 23, seed=10)
    chw = R.to_chw_f32(u8)
    t = torch.from_numpy(chw)
    m = torch.tensor(R.IMAGENET_MEAN, dtype=torch.float32)[:, None, None]
    s = torch.tensor(R.IMAGENET_STD, dtype=torch.float32)[:, None, None]
    assert np.array_equal(R.normalize(chw), ((t - m) / s).numpy())
    assert np.array_equal(chw, torch.from_numpy(u8.astype(np.float32) / 255.0).permute(2, 0, 1).numpy())


def test_flip_order():
    f = rnd(5, 7, seed=11)
    assert np.array_equal(R.flip(f, 3), f[::-1, ::-1])
    assert np.array_equal(R.flip(f, 1), f[:, ::-1]) and np.array_equal(R.flip(f, 2), f[::-1])


def test_golden_items_follow_the_restatement():
    """The fixture's items are resize -> flip -> /255 of the stored frames (the seeds' flips recovered here)."""
    z = np.load(GOLDEN)
    frames = {k[6:]: z[k] for k in z.files if k.startswith("frame_")}
    frames["hd_1080x1920"] = R.synth_frame(1080, 1920, 77)
    refs = {k[4:]: z[k] for k in z.files if k.startswith("ref_")}
    for group in ("dlp64", "dlp256", "vgg40", "vgg112", "vgg40_plain"):
        names, size, seed = list(z[f"{group}/names"]), int(z[f"{group}/size"]), int(z[f"{group}/seed"])
        flips = np.zeros(len(names), int)
        if seed >= 0:
            draws = np.random.RandomState(seed).rand(len(names), 2) > 0.5
            flips = draws[:, 0] * R.FLIP_LR + draws[:, 1] * R.FLIP_UD
        ri = 0
        for i, n in enumerate(names):
            assert np.array_equal(z[f"{group}/image"][i], R.flip(R.resize(frames[n], (size, size)), flips[i])), (group, n)
            if n in refs:
                assert np.array_equal(z[f"{group}/reference"][ri], R.flip(R.resize(refs[n], (size, size)), flips[i]))
                ri += 1
        assert ri == len(z[f"{group}/reference"])
    assert set(np.random.RandomState(int(z["vgg40/seed"])).rand(5, 2).__gt__(0.5).dot([1, 2])) == {0, 1, 2, 3}
    for name in ("odd_37x53", "hd_1080x1920", "area_128x128"):
        s = int(z[f"vgg/{name}/size"])
        want = R.normalize(R.to_chw_f32(R.resize(frames[name], (s, s))))[None]
        assert np.array_equal(z[f"vgg/{name}"], want), name
    for name in ("odd_37x53", "small_30x20"):
        assert np.array_equal(z[f"tensor/{name}"], R.to_chw_f32(frames[name])[None])
