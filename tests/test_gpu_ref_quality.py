"""uwie_reference_scores_u8 (MAE, MSE, PSNR, SSIM against a reference) and the best-of-N pick by them, on the device, against
the NumPy float64 statement of the definition (tests/ref_quality_ref.py) on the case table (tests/ref_quality_cases.py).

Tolerances.  mae and mse: none, the sums are integers and each column is one correctly rounded division.  psnr: 1e-9 relative
(one division and one logarithm of such a number).  SSIM: 1e-9 absolute on every column, derived, not measured: a window sum
of 121 weighted values <= 65025 carries at most a few 1e-11 of absolute float64 error in any order of summation and with or
without fused multiply-adds; var and cov inherit that; both factors of the denominator of s are at least C1 = 6.5 and C2 = 58.5,
the numerator's factors are bounded by the denominator's, so s moves by less than 1e-11, and the mean over the map does not
amplify.  1e-9 is the bound the underwater scores are held to.  Largest difference seen: 3.0e-14 on the flat pairs (var and cov are rounding residue there), 2.3e-15 on everything else
(README)."""
import ctypes
import math

import numpy as np
import pytest

import ref_quality_cases as K
import ref_quality_ref as ref

pytestmark = pytest.mark.gpu

TOL = 1e-9
E_INVALID, E_WORKSPACE = -1, -2  # include/uwie.h


@pytest.fixture(scope="module")
def uw():
    import underwater_image_enhancement_amd as uw

    return uw


@pytest.fixture(scope="module")
def dev(uw):
    d = uw.get_device(0)
    yield d
    # state after the calls: no kernel of this module left a bit in the device's status word
    assert d.check_status() == 0


@pytest.fixture(scope="module")
def tile():
    return K.plan(64, 64)


def close(got, want, what):
    """mae, mse bit for bit; psnr inf where it is inf, else 1e-9 relative; SSIM NaN exactly where there is no window, else
    1e-9 absolute."""
    got, want = np.asarray(got, np.float64).reshape(-1, 8), np.asarray(want, np.float64).reshape(-1, 8)
    assert got.shape == want.shape, what
    assert got[:, :2].tobytes() == want[:, :2].tobytes(), (what, got[:, :2].tolist(), want[:, :2].tolist())
    inf = np.isinf(want[:, 2])
    assert np.array_equal(np.isinf(got[:, 2]), inf) and np.all(got[inf, 2] > 0), (what, got[:, 2])
    dp, wp = np.abs(got[~inf, 2] - want[~inf, 2]), np.abs(want[~inf, 2])
    nan = np.isnan(want[:, 3:])
    assert np.array_equal(np.isnan(got[:, 3:]), nan), (what, got[:, 3:].tolist())
    err = np.abs(np.where(nan, 0.0, got[:, 3:] - want[:, 3:]))
    print(f"{what}: max |device - reference| psnr = {dp.max(initial=0.0):.3e}, SSIM = {err.max():.3e}")
    assert np.all(dp <= TOL * wp) and err.max() <= TOL, (what, got.tolist(), want.tolist())


def test_names(uw, tile):
    assert uw.REFERENCE_SCORE_NAMES == ref.NAMES and len(ref.NAMES) == 8
    assert tile[0] >= 1 and tile[1] >= 1


@pytest.fixture(scope="module")
def channel_ssims(tile):
    """The three channel SSIMs of every case of the table, which do not depend on gray_shift: computed once."""
    return {c.name: ref.channel_ssims(c.x, c.y) for c in K.shape_cases(tile)}


@pytest.mark.parametrize("gray_shift", [15, 14])
def test_every_case_equals_the_definition(dev, tile, channel_ssims, gray_shift):
    for c in K.shape_cases(tile):
        got = dev.reference_scores(dev.tensor(c.x[None]), dev.tensor(c.y[None]), gray_shift=gray_shift).cpu().numpy()[0]
        close(got, ref.scores(c.x, c.y, gray_shift, channels=channel_ssims[c.name]), f"{c.name} shift {gray_shift}")
        if c.name.startswith("identical"):  # exactly 0, 0, inf and, with a window, exactly 1.0
            assert got[:3].tolist() == [0.0, 0.0, math.inf], c.name
            assert np.all(got[3:] == 1.0) if c.has_window else np.all(np.isnan(got[3:])), (c.name, got)
        if c.name.startswith("opposite") and c.has_window:
            assert np.all(got[3:] < 0), (c.name, got)
        if c.name.startswith("flat") and c.has_window:
            for ch in range(3):
                a, b = float(c.x[0, 0, ch]), float(c.y[0, 0, ch])
                assert abs(got[4 + ch] - (2 * a * b + ref.C1) / (a * a + b * b + ref.C1)) <= TOL, c.name


@pytest.fixture(scope="module")
def full_hd():
    c = K.full_hd_case()
    return c, ref.channel_ssims(c.x, c.y)


@pytest.mark.parametrize("gray_shift", [15, 14])
def test_full_hd_pair(dev, full_hd, gray_shift):
    c, channels = full_hd
    x, y = dev.tensor(c.x[None]), dev.tensor(c.y[None])
    close(dev.reference_scores(x, y, gray_shift=gray_shift).cpu().numpy(), ref.scores(c.x, c.y, gray_shift, channels=channels),
          f"{c.name} shift {gray_shift}")
    if gray_shift == 15:  # identical at 1080p: exactly 1.0 over 2 million map points and 253 tiles
        assert dev.reference_scores(y, y).cpu().numpy()[0].tolist() == [0.0, 0.0, math.inf, 1.0, 1.0, 1.0, 1.0, 1.0]


def test_impulses_at_tile_seams_and_the_border(uw, tile):
    cases = K.impulse_cases(tile)
    got = uw.reference_scores(np.stack([c.x for c in cases]), cases[0].y)  # one reference for all
    assert got.shape == (len(cases), 8)
    want = np.array([ref.scores(c.x, c.y) for c in cases])
    close(got, want, "impulses")
    # the restatement tells the impulses apart (tests/test_ref_quality_cases.py), so the device does: same order, same gaps
    assert len(set(got[:, 3].tolist())) == len(cases) and np.array_equal(np.argsort(got[:, 3]), np.argsort(want[:, 3]))


def test_batch_equals_singles_bit_for_bit(uw, dev, tile):
    """Batches of strongly different pairs (K.batch_pairs) equal their single calls bit for bit: with a reference per frame,
    one reference for all, references shared by halves of a batch of 6, in two orders and twice over."""
    xs, ys = K.batch_pairs(tile)
    single = np.stack([uw.reference_scores(x, y) for x, y in zip(xs, ys)])
    assert single.shape == (3, 8)
    close(single, np.array([ref.scores(x, y) for x, y in zip(xs, ys)]), "batch pairs alone")
    for order in ([0, 1, 2], [2, 1, 0]):
        for _ in range(2):  # ref_batch = batch, the same call twice
            assert uw.reference_scores(xs[order], ys[order]).tobytes() == single[order].tobytes(), order
    # ref_batch = 1: every frame against reference 1, as a frame and as a batch of one
    against1 = np.stack([uw.reference_scores(x, ys[1]) for x in xs])
    assert uw.reference_scores(xs, ys[1]).tobytes() == against1.tobytes() == uw.reference_scores(xs, ys[1:2]).tobytes()
    assert against1[1].tobytes() == single[1].tobytes() and against1[0].tobytes() != single[0].tobytes()
    # ref_batch = batch / 2 on a batch of 6: frame i against reference i % 3
    six = np.concatenate([xs, xs[[1, 2, 0]]])
    want6 = np.stack([uw.reference_scores(six[i], ys[i % 3]) for i in range(6)])
    got6 = dev.reference_scores(dev.tensor(six), dev.tensor(ys))
    assert got6.is_cuda and tuple(got6.shape) == (6, 8) and got6.cpu().numpy().tobytes() == want6.tobytes()
    assert want6[:3].tobytes() == single.tobytes()
    # a device tensor comes back as a device tensor of the same numbers; a single frame gives (8,)
    t = uw.reference_scores(dev.tensor(xs), dev.tensor(ys))
    assert t.is_cuda and tuple(t.shape) == (3, 8) and t.cpu().numpy().tobytes() == single.tobytes()
    assert uw.reference_scores(dev.tensor(xs[1]), ys[1]).shape == (8,)


def test_quality_class_and_float_images(uw, tile):
    xs, ys = K.batch_pairs(tile)
    want = ref.scores(xs[0], ys[0])
    d = uw.ReferenceQuality.scores(xs[0], ys[0])
    assert list(d) == list(ref.NAMES)
    close(np.array([d[k] for k in ref.NAMES]), want, "ReferenceQuality.scores")
    assert uw.ReferenceQuality.psnr(xs[0], ys[0]) == d["psnr"]
    assert uw.ReferenceQuality.ssim(xs[0], ys[0]) == d["ssim_y"] == uw.ReferenceQuality.ssim(xs[0], ys[0], channels="y")
    assert uw.ReferenceQuality.ssim(xs[0], ys[0], channels="rgb") == d["ssim_rgb"]
    rng = np.random.default_rng(3)
    a = rng.random((40, 56, 3))  # float images: (x * 255).astype(uint8) is what is scored
    b = np.clip(a + rng.normal(0, 0.05, a.shape), 0, 1)
    got = uw.ReferenceQuality.scores(a, (b * 255).astype(np.uint8))
    close(np.array([got[k] for k in ref.NAMES]), ref.scores((a * 255).astype(np.uint8), (b * 255).astype(np.uint8)), "float image")
    import torch

    assert uw.ReferenceQuality.psnr(torch.from_numpy(a), torch.from_numpy(b)) == got["psnr"]
    with pytest.raises(ValueError):
        uw.ReferenceQuality.scores(np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8))
    with pytest.raises(ValueError):
        uw.ReferenceQuality.ssim(xs[0], ys[0], channels="r")


def test_workspace_and_argument_guards(uw, dev, tile):
    import torch

    lib = dev.lib
    xs, ys = K.batch_pairs(tile)
    six, refs = dev.tensor(np.concatenate([xs, xs])), dev.tensor(ys)
    B, H, W = six.shape[:3]
    need = lib.uwie_workspace_bytes_reference(B, H, W)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev.torch_device)
    out = torch.empty((B, 8), dtype=torch.float64, device=dev.torch_device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    call = lambda *a: lib.uwie_reference_scores_u8(dev._ctx, *a, dev.stream())  # noqa: E731
    assert call(p(six), p(refs), B, 3, H, W, 15, p(out), p(ws), need) == 0  # the stated size suffices
    assert out.cpu().numpy().tobytes() == dev.reference_scores(six, refs).cpu().numpy().tobytes()
    assert call(p(six), p(refs), B, 3, H, W, 15, p(out), p(ws), need - 1) == E_WORKSPACE
    assert call(p(six), p(refs), B, 3, H, W, 15, p(out), None, need) == E_WORKSPACE
    assert call(None, p(refs), B, 3, H, W, 15, p(out), p(ws), need) == E_INVALID
    assert call(p(six), None, B, 3, H, W, 15, p(out), p(ws), need) == E_INVALID
    assert call(p(six), p(refs), B, 3, H, W, 15, None, p(ws), need) == E_INVALID
    assert call(p(six), p(refs), B, 3, 0, W, 15, p(out), p(ws), need) == E_INVALID
    assert call(p(six), p(refs), B, 3, H, W, 13, p(out), p(ws), need) == E_INVALID
    for bad in (0, -1, 4, 5, 7, 12):  # ref_batch must be 1 .. batch and divide it
        assert call(p(six), p(refs), B, bad, H, W, 15, p(out), p(ws), need) == E_INVALID, bad
    assert call(p(six), p(refs), 65536, 1, H, W, 15, p(out), p(ws), need) == E_INVALID
    assert lib.uwie_reference_scores_u8(None, p(six), p(refs), B, 3, H, W, 15, p(out), p(ws), need, dev.stream()) == E_INVALID
    with pytest.raises(TypeError):
        uw.reference_scores(np.zeros((8, 8, 3), np.float32), np.zeros((8, 8, 3), np.uint8))
    with pytest.raises(ValueError):
        uw.reference_scores(np.zeros((8, 8, 4), np.uint8), np.zeros((8, 8, 4), np.uint8))
    with pytest.raises(ValueError):  # another size
        uw.reference_scores(np.zeros((12, 12, 3), np.uint8), np.zeros((12, 13, 3), np.uint8))
    with pytest.raises(ValueError):  # two references for three frames
        uw.reference_scores(xs, ys[:2])
    with pytest.raises(ValueError):
        dev.reference_scores(six[:5], refs)


@pytest.fixture(scope="module")
def selection(uw):
    """The frames and references, every strategy's device output, and the restatement's scores of those outputs [n, B, 8]:
    computed once."""
    frames, refs = K.selection_frames()
    _, _, _, every = uw.select_best(frames, return_all=True)
    names = [uw.CONFIG_STRATEGIES[k]["name"] for k in uw.CONFIG_STRATEGIES]
    want = np.array([[ref.scores(every[name][b], refs[b]) for b in range(len(frames))] for name in names])
    return frames, refs, names, every, want


@pytest.mark.parametrize("metric", ["psnr", "ssim_y", "ssim_rgb"])
def test_select_best_reference_equals_the_loop(uw, selection, metric):
    frames, refs, names, every, want = selection
    col = ref.NAMES.index(metric)
    best_names, images, scores, outs = uw.select_best_reference(frames, refs, metric=metric, return_all=True)
    assert scores.shape == (len(names), len(frames), 8) and scores.dtype == np.float64 and list(outs) == names
    close(scores, want, f"select_best_reference {metric}")
    for b in range(len(frames)):
        ranked = np.sort(want[:, b, col])[::-1]
        assert ranked[0] - ranked[1] > 1e-6, (b, ranked)  # the cases file chose frames with a clear winner
        k = int(np.argmax(want[:, b, col]))
        assert best_names[b] == names[k], (b, best_names[b], names[k])
        assert np.array_equal(images[b], every[names[k]][b]) and np.array_equal(outs[names[k]][b], every[names[k]][b])
    # a single frame: a name, an image, scores with B = 1
    name1, img1, sc1 = uw.select_best_reference(frames[0], refs[0], metric=metric)
    assert name1 == best_names[0] and np.array_equal(img1, images[0]) and sc1.tobytes() == scores[:, :1].tobytes()


def test_one_reference_for_all_frames(uw, selection):
    frames, refs, names, every, want = selection
    best_names, images, scores = uw.select_best_reference(frames, refs[1])
    assert scores[:, 1].tobytes() == uw.select_best_reference(frames, refs)[2][:, 1].tobytes()
    assert best_names[1] == names[int(np.argmax(want[:, 1, 3]))]
    close(scores[:, 0], np.array([ref.scores(every[name][0], refs[1]) for name in names]), "frame 0 against reference 1")


@pytest.mark.parametrize("metric", ["psnr", "ssim_y", "ssim_rgb"])
def test_the_first_of_two_equal_sets_wins(uw, selection, metric):
    """One call with frame 0's winner listed twice (a list of pairs: a dict cannot hold a key twice) behind a set that loses
    to it: the two score the same bits, and the first of them is picked."""
    frames, refs, names, every, want = selection
    keys = list(uw.CONFIG_STRATEGIES)
    k = int(np.argmax(want[:, 0, ref.NAMES.index(metric)]))
    win, lose = keys[k], keys[(k + 1) % len(keys)]
    pairs = [(lose, uw.CONFIG_STRATEGIES[lose]), (win, {**uw.CONFIG_STRATEGIES[win], "name": "First"}),
             (win, {**uw.CONFIG_STRATEGIES[win], "name": "Second"})]
    best, image, scores = uw.select_best_reference(frames[0], refs[0], strategies=pairs, metric=metric)
    assert scores.shape == (3, 1, 8) and scores[1].tobytes() == scores[2].tobytes()
    assert best == "First" and np.array_equal(image, every[names[k]][0])


def test_unknown_metric_and_strategy_are_errors(uw):
    frames, refs = K.selection_frames()
    for metric in ("mse", "mae", "ssim_r", "uiqm"):  # smaller is better, or not a column of this table
        with pytest.raises(ValueError, match=metric):
            uw.select_best_reference(frames[0], refs[0], metric=metric)
    with pytest.raises(ValueError):
        uw.select_best_reference(frames[0], refs[0], strategies={"no_such_strategy": {}})
