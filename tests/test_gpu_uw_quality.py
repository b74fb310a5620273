"""uwie_underwater_scores_u8 (UCIQE, UIQM) and the best-of-N pick by them, on the device, against the NumPy float64
statement of the definition (tests/uw_quality_ref.py) on the case table (tests/uw_quality_cases.py).

Tolerance: 1e-9 absolute on every score, the bound the project already holds integer-derived scores to against a float64
evaluation (uwie_quality_scores, tests/quality_ref.py).  con_l, UICM's moments and every block's extrema are exact integers on
both sides; what differs is the order of float64 sums (n <= 2.1e6 terms below 1, a relative 1e-13 at the very most) and the
last bit of a logarithm or a square root.  sigma_c's sums are shifted by a value of the frame (k_uw_quality.hip), so its
cancellation stays below 1e-12 as well; nothing here needed more than 1e-9."""
import ctypes

import numpy as np
import pytest

import uw_quality_cases as K
import uw_quality_ref as ref

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
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == np.float64 and got.shape == want.shape, what
    err = np.abs(got - want)
    worst = ref.NAMES[int(np.argmax(err.reshape(-1, 8).max(axis=0)))] if err.ndim else ""
    print(f"{what}: max |device - reference| = {err.max():.3e} {worst}")
    assert np.all(err <= TOL), (what, got.tolist(), want.tolist())


def test_names_and_plan(uw, tile):
    assert uw.UNDERWATER_SCORE_NAMES == ref.NAMES and len(ref.NAMES) == 8
    assert tile[0] % 8 == 0 and tile[1] % 8 == 0


@pytest.mark.parametrize("gray_shift", [15, 14])
def test_every_case_equals_the_definition(uw, dev, tile, gray_shift):
    for c in K.shape_cases(tile):
        got = dev.underwater_scores(dev.tensor(c.frame[None]), gray_shift=gray_shift).cpu().numpy()[0]
        close(got, ref.scores(c.frame, gray_shift), f"{c.name} shift {gray_shift}")
        if c.name.startswith(("flat_gray", "black", "white")):
            assert np.all(got == 0.0), c.name  # one gray level scores 0 everywhere
        if c.name.startswith("flat_colour"):
            assert got[0] == 0.0 and got[2] > 0.0, c.name  # sigma_c of one colour is exactly 0, mu_s is not


def test_full_hd_frame(uw):
    c = K.full_hd_case()
    close(uw.underwater_scores(c.frame), ref.scores(c.frame), c.name)


def test_impulses_at_block_seams_tile_seams_and_the_border(uw, tile):
    cases = K.impulse_cases(tile)
    got = uw.underwater_scores(np.stack([c.frame for c in cases]))
    assert got.shape == (len(cases), 8)
    for row, c in zip(got, cases):
        close(row, ref.scores(c.frame), c.name)


def test_batch_equals_singles_bit_for_bit(uw, dev, tile):
    """A batch of three different frames equals its three single calls bit for bit, in two orders and twice over.  The middle
    frame is a dark ramp between two bright ones (K.batch_frames): on constant black and white frames q = gradient * value
    is zero on one side of every border, so a halo row read from the neighbouring frame could not show; on these it does
    (tests/test_uw_quality_cases.py proves that on the reference)."""
    frames = K.batch_frames(tile)
    single = np.stack([uw.underwater_scores(f) for f in frames])
    assert single.shape == (3, 8)
    for f, row in zip(frames, single):
        close(row, ref.scores(f), "batch frame alone")
    for order in ((0, 1, 2), (2, 1, 0)):
        for _ in range(2):
            got = uw.underwater_scores(frames[list(order)])
            assert got.tobytes() == single[list(order)].tobytes(), order
    # a device tensor comes back as a device tensor of the same numbers; a single frame gives (8,)
    t = uw.underwater_scores(dev.tensor(frames))
    assert t.is_cuda and tuple(t.shape) == (3, 8) and t.cpu().numpy().tobytes() == single.tobytes()
    assert uw.underwater_scores(dev.tensor(frames[1])).shape == (8,)


def test_quality_class_and_float_images(uw):
    f = K.batch_frames(K.plan(64, 64))[0]
    want = ref.scores(f)
    d = uw.UnderwaterQuality.scores(f)
    assert list(d) == list(ref.NAMES)
    close(np.array([d[k] for k in ref.NAMES]), want, "UnderwaterQuality.scores")
    assert uw.UnderwaterQuality.uciqe(f) == d["uciqe"] and uw.UnderwaterQuality.uiqm(f) == d["uiqm"]
    x = np.random.default_rng(3).random((40, 56, 3))  # a float image: (x * 255).astype(uint8) is what is scored
    close(uw.UnderwaterQuality.uiqm(x), ref.scores((x * 255).astype(np.uint8))[7], "float image")
    with pytest.raises(ValueError):
        uw.UnderwaterQuality.scores(np.zeros((8, 8), np.uint8))


def test_workspace_and_argument_guards(uw, dev):
    import torch

    lib = dev.lib
    frames = dev.tensor(K.batch_frames(K.plan(64, 64)))
    B, H, W = frames.shape[:3]
    need = lib.uwie_workspace_bytes_underwater(B, H, W)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev.torch_device)
    out = torch.empty((B, 8), dtype=torch.float64, device=dev.torch_device)
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    call = lambda *a: lib.uwie_underwater_scores_u8(dev._ctx, *a, dev.stream())  # noqa: E731
    assert call(p(frames), B, H, W, 15, p(out), p(ws), need) == 0  # the stated size suffices
    assert out.cpu().numpy().tobytes() == dev.underwater_scores(frames).cpu().numpy().tobytes()
    assert call(p(frames), B, H, W, 15, p(out), p(ws), need - 1) == E_WORKSPACE
    assert call(p(frames), B, H, W, 15, p(out), None, need) == E_WORKSPACE
    assert call(None, B, H, W, 15, p(out), p(ws), need) == E_INVALID
    assert call(p(frames), B, H, W, 15, None, p(ws), need) == E_INVALID
    assert call(p(frames), B, 0, W, 15, p(out), p(ws), need) == E_INVALID
    assert call(p(frames), 65536, H, W, 15, p(out), p(ws), need) == E_INVALID
    assert call(p(frames), B, H, W, 13, p(out), p(ws), need) == E_INVALID
    assert lib.uwie_underwater_scores_u8(None, p(frames), B, H, W, 15, p(out), p(ws), need, dev.stream()) == E_INVALID
    # the pick: NULL pointers, a column outside the row, outputs given by halves
    sc = torch.zeros((2, B, 8), dtype=torch.float64, device=dev.torch_device)
    best = torch.empty((B,), dtype=torch.int32, device=dev.torch_device)
    pick = lambda *a: lib.uwie_pick_best_u8(dev._ctx, *a, dev.stream())  # noqa: E731
    assert pick(None, 2, B, 8, 7, None, 0, 0, p(best), None) == E_INVALID
    assert pick(p(sc), 2, B, 8, 7, None, 0, 0, None, None) == E_INVALID
    assert pick(p(sc), 2, B, 8, 8, None, 0, 0, p(best), None) == E_INVALID
    assert pick(p(sc), 0, B, 8, 7, None, 0, 0, p(best), None) == E_INVALID
    assert pick(p(sc), 2, B, 8, 7, p(frames), H, W, p(best), None) == E_INVALID
    assert pick(p(sc), 2, B, 8, 7, None, 0, 0, p(best), None) == 0
    assert best.cpu().tolist() == [0] * B  # all equal: the first set wins
    with pytest.raises(TypeError):
        uw.underwater_scores(np.zeros((8, 8, 3), np.float32))
    with pytest.raises(ValueError):
        uw.underwater_scores(np.zeros((8, 8, 4), np.uint8))


def test_pick_best_takes_the_first_maximum_of_any_column(dev):
    import torch

    rng = np.random.default_rng(12)
    sc = rng.integers(0, 4, (5, 7, 3)).astype(np.float64)  # many ties
    every = rng.integers(0, 256, (5, 7, 9, 11, 3), dtype=np.uint8)
    for col in range(3):
        best, img = dev.pick_best_u8(dev.tensor(sc), col, dev.tensor(every))
        want = np.argmax(sc[:, :, col], axis=0)  # np.argmax: the first maximum
        assert best.cpu().tolist() == want.tolist(), col
        assert np.array_equal(img.cpu().numpy(), every[want, np.arange(7)])
        assert torch.equal(dev.pick_best_u8(dev.tensor(sc), col)[0], best)


@pytest.fixture(scope="module")
def selection(uw):
    """The frames, every strategy's device output, and the reference's scores of those outputs [n, B, 8]: computed once."""
    frames = K.selection_frames()
    _, _, _, every = uw.select_best(frames, return_all=True)
    names = [uw.CONFIG_STRATEGIES[k]["name"] for k in uw.CONFIG_STRATEGIES]
    want = np.array([[ref.scores(every[name][b]) for b in range(len(frames))] for name in names])
    return frames, names, every, want


@pytest.mark.parametrize("metric", ["uiqm", "uciqe"])
def test_select_best_underwater_equals_the_loop(uw, selection, metric):
    frames, names, every, want = selection
    col = ref.NAMES.index(metric)
    best_names, images, scores, outs = uw.select_best_underwater(frames, metric=metric, return_all=True)
    assert scores.shape == (len(names), len(frames), 8) and scores.dtype == np.float64 and list(outs) == names
    close(scores, want, f"select_best_underwater {metric}")
    for b in range(len(frames)):
        ranked = np.sort(want[:, b, col])[::-1]
        assert ranked[0] - ranked[1] > 1e-6, (b, ranked)  # the cases file chose frames with a clear winner
        k = int(np.argmax(want[:, b, col]))
        assert best_names[b] == names[k], (b, best_names[b], names[k])
        assert np.array_equal(images[b], every[names[k]][b]) and np.array_equal(outs[names[k]][b], every[names[k]][b])
    # a single frame: a name, an image, scores with B = 1
    name1, img1, sc1 = uw.select_best_underwater(frames[0], metric=metric)
    assert name1 == best_names[0] and np.array_equal(img1, images[0]) and sc1.tobytes() == scores[:, :1].tobytes()


@pytest.mark.parametrize("metric", ["uiqm", "uciqe"])
def test_the_first_of_two_equal_sets_wins(uw, selection, metric):
    """One call with frame 0's winner listed twice (a list of pairs: a dict cannot hold a key twice) behind a set that loses
    to it: the two score the same bits, and the first of them is picked."""
    frames, names, every, want = selection
    keys = list(uw.CONFIG_STRATEGIES)
    k = int(np.argmax(want[:, 0, ref.NAMES.index(metric)]))
    win, lose = keys[k], keys[(k + 1) % len(keys)]
    pairs = [(lose, uw.CONFIG_STRATEGIES[lose]), (win, {**uw.CONFIG_STRATEGIES[win], "name": "First"}),
             (win, {**uw.CONFIG_STRATEGIES[win], "name": "Second"})]
    best, image, scores = uw.select_best_underwater(frames[0], strategies=pairs, metric=metric)
    assert scores.shape == (3, 1, 8) and scores[1].tobytes() == scores[2].tobytes()
    assert best == "First" and np.array_equal(image, every[names[k]][0])


def test_unknown_metric_and_strategy_are_errors(uw):
    f = K.selection_frames()[0]
    with pytest.raises(ValueError, match="psnr"):
        uw.select_best_underwater(f, metric="psnr")
    with pytest.raises(ValueError):
        uw.select_best_underwater(f, strategies={"no_such_strategy": {}})
