"""EndToEndTrainer's training step on the device (uwie_mlp_trainer_*, uw.EndToEndTrainer): the train-mode
forward, the MLP's backward, clip_grad_norm_ and Adam against the real trainer's records (tests/golden/mlp_train.npz) and the
float64 restatement (tests/mlp_train_ref.py), within DEVICE_MARGIN times the restatement's own measured distance from the
real trainer (tests/test_mlp_train_ref.py)."""
import numpy as np
import pytest

import gated_predictor_ref as R
import mlp_train_ref as T

pytestmark = pytest.mark.gpu

M = T.DEVICE_MARGIN


@pytest.fixture(scope="module")
def dev():
    import underwater_image_enhancement_amd as uw

    return uw.get_device(0)


@pytest.fixture(scope="module")
def gold():
    return T.load_golden()


@pytest.fixture(scope="module")
def state0():
    return R.small_state(R.load_golden())


@pytest.fixture(scope="module")
def big():
    return R.seeded_state(int(R.load_golden()["seed"]))


def trainer(state, **kw):
    import underwater_image_enhancement_amd as uw

    return uw.EndToEndTrainer({k: v.copy() for k, v in state.items()}, **kw)


def bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return a.view(np.int32 if a.dtype == np.float32 else np.uint8)


def same_bits(a, b):
    return all(np.array_equal(bits(a[k]), bits(b[k])) for k in a)


def host(d):
    return {k: v.numpy() for k, v in d.items()}


def batch(dev, gold, i):
    img = gold[f"batch/{i}/u8"].astype(np.float32) / np.float32(255.0)
    return dev.tensor(img), dev.tensor(gold[f"batch/{i}/reference"]), dev.tensor(gold[f"batch/{i}/features"])


def manual_step(dev, tr, img, ref, rows, masks, nan_columns=True):
    """train_step's entry points called one by one: (cols, loss, l1, l2, the gradients before the clip)"""
    from underwater_image_enhancement_amd import _lib
    from underwater_image_enhancement_amd.modules import _read_loss

    ws = dev.mlp_train_workspace(rows.shape[0], tr.hidden_dim, tr.num_blocks)
    cols = dev.mlp_train_forward(tr._handle, rows, ws, tr.dropout, masks, tr.seed)
    _, saved, buf = dev.ref_loss_f32(_lib.LOSS_GATED, img, cols, ref, True, status=True)
    _, gcols = dev.ref_loss_bwd_f32(_lib.LOSS_GATED, img, cols, saved, ref, tr._grad_loss, True, want_img=False)
    if nan_columns:  # the first two columns carry nothing the backward may read
        gcols = gcols.clone()
        gcols[:, :2] = float("nan")
    dev.mlp_backward(tr._handle, rows, ws, gcols)
    grads = host(tr.gradients())
    dev.mlp_adam_step(tr._handle, tr.lr, tr.betas, tr.eps, tr.max_norm)
    l1, l2 = _read_loss(dev, buf, img, cols)
    loss = float(np.float32(0.5) * np.float32(l1) + np.float32(0.5) * np.float32(l2))
    return cols.cpu().numpy(), loss, l1, l2, grads


def dev_masks(dev, m):
    return dev.tensor(np.ascontiguousarray(m, dtype=np.uint8))


# ---------------------------------------------------------------- p = 0
@pytest.mark.parametrize("net", ["small", "big"])
def test_p0_is_the_eval_forward_bit_for_bit(dev, state0, big, net):
    import torch

    import underwater_image_enhancement_amd as uw

    state = state0 if net == "small" else big
    tr, model = trainer(state, dropout=0.0), uw.ParameterPredictor(state)
    rows = np.random.default_rng(11).standard_normal((70, 79)) * 2.0
    for B in (1, 3, 70):
        r = dev.tensor(rows[:B])  # float64 rows, rounded on load
        want = bits(model.columns(rows[:B]))
        ws = dev.mlp_train_workspace(B, tr.hidden_dim, tr.num_blocks)
        assert np.array_equal(bits(dev.mlp_train_forward(tr._handle, r, ws, 0.0)), want), B  # drawn, nothing to draw
        none = torch.zeros((T.sites(tr.num_blocks), B, tr.hidden_dim), dtype=torch.uint8, device=dev.torch_device)
        assert np.array_equal(bits(dev.mlp_train_forward(tr._handle, r, ws, 0.0, none)), want), B  # p = 0: no site acts
        assert np.array_equal(bits(dev.mlp_train_forward(tr._handle, r.float(), ws, 0.0)), want), B
        assert np.array_equal(bits(tr.param_predictor.columns(rows[:B])), want), B  # uwie_mlp_trainer_eval
    got = tr.param_predictor(rows[:3])
    assert list(got) == list(R.HEADS) and all(tuple(v.shape) == (3, 1) for v in got.values())
    tr.close()
    model.close()


# ---------------------------------------------------------------- the real trainer's records
@pytest.fixture(scope="module")
def run_a(dev, gold, state0):
    """case A's four steps through the entry points one by one, with the golden masks"""
    tr = trainer(state0)
    steps = []
    for s in range(4):
        img, ref, feat = batch(dev, gold, s)
        steps.append(manual_step(dev, tr, img, ref, feat, dev_masks(dev, gold[f"a/{s}/masks"])))
    end = host(tr.state_dict())
    tr.close()
    return steps, end


def test_given_masks_against_the_goldens(gold, state0, run_a):
    steps, end = run_a
    span = np.array([R.SPAN[k] for k in R.GATED_ORDER])
    for s, (cols, loss, l1, l2, grads) in enumerate(steps):
        want = R.columns({k: gold[f"a/{s}/{k}"] for k in R.HEADS})
        e_cols = float((np.abs(cols - want) / span).max())
        assert e_cols <= R.DEVICE_TOL, (s, e_cols)
        worst = 0.0
        for k in state0:
            if k in T.FREE:
                assert not grads[k].any(), (s, k)  # exact zeros, with NaN in d_grad_out's first two columns
                continue
            g = gold[f"a/{s}/grad/{k}"]
            assert not grads[k][g == 0].any(), (s, k)  # golden zeros are zeros
            assert np.isfinite(grads[k]).all()
            worst = max(worst, T.grad_error(grads[k], g))
        print(f"step {s}: heads {e_cols:.3g} of the range, gradients {worst:.3g} (tolerance {M * T.REF_GRAD_ERROR:.3g}), "
              f"loss off by {abs(loss - float(gold[f'a/{s}/loss'])):.3g}")
        assert worst <= M * T.REF_GRAD_ERROR, s
        for got, key in ((loss, "loss"), (l1, "l1"), (l2, "l2")):
            assert abs(got - float(gold[f"a/{s}/{key}"])) <= M * T.REF_TRAJ_ERROR[1], (s, key)
    e_par = max(float(np.abs(end[k].astype(np.float64) - gold[f"a/after4/param/{k}"]).max()) for k in state0)
    print(f"parameters after four steps: off by {e_par:.3g} (tolerance {M * T.REF_TRAJ_ERROR[0]:.3g})")
    assert e_par <= M * T.REF_TRAJ_ERROR[0]
    assert all(np.array_equal(bits(end[k]), bits(state0[k])) for k in T.FREE)


def test_train_step_is_its_entry_points(dev, gold, state0, run_a):
    steps, end = run_a
    tr = trainer(state0)
    for s in range(4):
        img, ref, feat = batch(dev, gold, s)
        loss, parts = tr.train_step(img, ref, feat, masks=gold[f"a/{s}/masks"])
        assert isinstance(loss, float) and sorted(parts) == ["l1", "l2"]
        assert (loss, parts["l1"], parts["l2"]) == steps[s][1:4], s
    assert tr.step_count == 4 and same_bits(host(tr.state_dict()), end)
    tr.close()


def test_train_epoch_averages_its_steps(dev, gold, state0):
    data = []
    for i in range(2):
        img, ref, feat = batch(dev, gold, i)
        data.append({"image": img, "reference": ref, "features": feat})
    one, two = trainer(state0, seed=5), trainer(state0, seed=5)
    parts = [one.train_step(b["image"], b["reference"], b["features"]) for b in data]
    avg, avgs = two.train_epoch(data)
    assert avg == (parts[0][0] + parts[1][0]) / 2
    assert avgs == {k: (parts[0][1][k] + parts[1][1][k]) / 2 for k in ("l1", "l2")}
    assert same_bits(host(one.state_dict()), host(two.state_dict()))
    # validate is the eval forward's loss, averaged the same way; features None: FeatureExtractor's rows
    v, vp = two.validate(data)
    each = [two.validate_batch(b["image"], b["reference"], b["features"]) for b in data]
    assert v == (each[0][0] + each[1][0]) / 2 and vp["l1"] == (each[0][1]["l1"] + each[1][1]["l1"]) / 2
    loss, _ = two.train_step(data[0]["image"], data[0]["reference"])
    assert np.isfinite(loss)
    one.close()
    two.close()


# ---------------------------------------------------------------- the float64 restatement, shapes no fixture holds
@pytest.mark.parametrize("dims,B", [((79, 64, 1), 1), ((79, 256, 3), 70), ((5, 6, 0), 3), ((79, 1152, 1), 2)])
def test_against_the_float64_restatement(dev, dims, B):
    F, H, nb = dims
    state = R.seeded_state(31 + H, F, H, nb)
    rng = np.random.default_rng(H * 100 + B)
    rows = rng.standard_normal((B, F))
    masks = (rng.random((T.sites(nb), B, H)) >= T.P_DROP).astype(np.uint8)
    gh = {"use_gamma": rng.standard_normal((B, 1)), "gamma": rng.standard_normal((B, 1))}
    gcols = np.full((B, 4), np.nan, dtype=np.float32)
    gcols[:, 2], gcols[:, 3] = gh["use_gamma"][:, 0], gh["gamma"][:, 0]
    gh = {"use_gamma": gcols[:, 2:3].astype(np.float64), "gamma": gcols[:, 3:4].astype(np.float64)}
    out64, cache = T.forward64(state, rows, masks)
    g64 = T.backward64(state, cache, gh)

    tr = trainer(state)
    r, m, g = dev.tensor(rows), dev_masks(dev, masks), dev.tensor(gcols)
    ws = dev.mlp_train_workspace(B, H, nb)
    cols = dev.mlp_train_forward(tr._handle, r, ws, T.P_DROP, m).cpu().numpy()
    span = np.array([R.SPAN[k] for k in R.GATED_ORDER])
    e_cols = float((np.abs(cols - R.columns(out64)) / span).max())
    dev.mlp_backward(tr._handle, r, ws, g)
    grads = host(tr.gradients())
    worst = 0.0
    for k in state:
        assert np.isfinite(grads[k]).all(), k
        assert not grads[k][g64[k] == 0].any(), k
        if k not in T.FREE:
            worst = max(worst, T.grad_error(grads[k], g64[k]))
    print(f"{dims}, B = {B}: heads {e_cols:.3g} of the range, gradients {worst:.3g} (tolerance {M * T.REF_GRAD_ERROR:.3g})")
    assert e_cols <= R.DEVICE_TOL and worst <= M * T.REF_GRAD_ERROR
    # deterministic: a second forward and backward give the same bits
    cols2 = dev.mlp_train_forward(tr._handle, r, ws, T.P_DROP, m).cpu().numpy()
    dev.mlp_backward(tr._handle, r, ws, g)
    assert np.array_equal(bits(cols), bits(cols2)) and same_bits(grads, host(tr.gradients()))
    if B > 1:  # dW is the batch's sum: the first row alone gives something else
        _, c1 = T.forward64(state, rows[:1], masks[:, :1])
        g1 = T.backward64(state, c1, {k: v[:1] for k, v in gh.items()})
        assert T.grad_error(grads["output_proj.0.weight"], g1["output_proj.0.weight"]) > 100 * M * T.REF_GRAD_ERROR
    tr.close()


# ---------------------------------------------------------------- clip and Adam
def feed(tr, gold, tag, state0, free_value=0.0):
    tr._set(1, {k: gold[f"{tag}/grad/{k}"] if k not in T.FREE else np.full_like(state0[k], free_value) for k in state0})


def check_snapshot(tr, gold, tag, state0):
    from underwater_image_enhancement_amd import _lib

    worst = 0.0
    for which, name in ((_lib.TRAINER_PARAMS, "param"), (_lib.TRAINER_EXP_AVG, "exp_avg"), (_lib.TRAINER_EXP_AVG_SQ, "exp_avg_sq")):
        got = host(tr._array(which))
        for k in state0:
            if k in T.FREE:
                want = state0[k] if name == "param" else np.zeros_like(state0[k])
                assert np.array_equal(bits(got[k]), bits(want)), (tag, name, k)  # unchanged to the bit
            else:
                worst = max(worst, T.ulps(got[k], gold[f"{tag}/{name}/{k}"]))
    print(f"{tag}: {worst:.3g} ulp (tolerance {M * T.REF_ADAM_ERROR:.3g})")
    assert worst <= M * T.REF_ADAM_ERROR, tag


def test_clip_and_adam_fed_the_golden_gradients(dev, gold, state0):
    import torch

    norm = torch.zeros(1, dtype=torch.float64, device=dev.torch_device)
    for case, steps, max_norm, marks in (("a", 4, 1.0, {1: "a/after1", 4: "a/after4"}), ("b", 2, float(gold["b/max_norm"]), {2: "b/after2"})):
        tr = trainer(state0, max_norm=max_norm)
        for s in range(steps):
            feed(tr, gold, f"{case}/{s}", state0, free_value=1e3)  # the gradient-free heads are outside the norm and the update
            dev.mlp_adam_step(tr._handle, tr.lr, tr.betas, tr.eps, tr.max_norm, norm)
            want = T.total_norm64({k: gold[f"{case}/{s}/grad/{k}"] for k in state0 if k not in T.FREE})
            assert abs(float(norm.item()) - want) <= 1e-6 * want, (case, s)
            assert (want > max_norm) == (case == "b")
            if s + 1 in marks:
                check_snapshot(tr, gold, marks[s + 1], state0)
        assert tr.step_count == steps
        tr.close()


def test_a_nan_gradient_reaches_every_updated_parameter(dev, gold, state0):
    tr = trainer(state0)
    grads = {k: gold[f"a/0/grad/{k}"].copy() if k not in T.FREE else np.zeros_like(state0[k]) for k in state0}
    grads["res_blocks.0.block.3.bias"][5] = np.nan
    tr._set(1, grads)
    dev.mlp_adam_step(tr._handle, tr.lr, tr.betas, tr.eps, tr.max_norm)
    end = host(tr.state_dict())
    for k in state0:
        if k in T.FREE:
            assert np.array_equal(bits(end[k]), bits(state0[k])), k
        else:
            assert np.isnan(end[k]).all(), k
    tr.close()


# ---------------------------------------------------------------- checkpoints
def golden_checkpoint(gold, state0, tag, with_free):
    import torch

    state = {}
    for i, k in enumerate(state0):
        if k not in T.FREE:
            state[i] = {"step": torch.tensor(float(gold[f"{tag}/step"])), "exp_avg": torch.from_numpy(gold[f"{tag}/exp_avg/{k}"].copy()),
                        "exp_avg_sq": torch.from_numpy(gold[f"{tag}/exp_avg_sq/{k}"].copy())}
        elif with_free:
            state[i] = {"step": torch.tensor(float(gold[f"{tag}/step"])), "exp_avg": torch.zeros(state0[k].shape),
                        "exp_avg_sq": torch.zeros(state0[k].shape)}
    group = {"lr": 1e-4, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False, "params": list(range(len(state0)))}
    return {"param_predictor": {k: torch.from_numpy(gold[f"{tag}/param/{k}"].copy()) for k in state0},
            "optimizer": {"state": state, "param_groups": [group]}}


def test_resume(dev, gold, state0, tmp_path):
    import torch

    def steps(tr, which):
        for s in which:
            img, ref, feat = batch(dev, gold, s)
            tr.train_step(img, ref, feat, masks=gold[f"a/{s}/masks"])

    # the uninterrupted run writes a checkpoint after step 1; a second trainer resumes from it: the same end, bit for bit
    whole = trainer(state0)
    steps(whole, [0])
    path = tmp_path / "ckpt.pth"
    whole.save_model(path)
    steps(whole, [1, 2, 3])
    resumed = trainer(state0)
    resumed.load_model(path)
    assert resumed.step_count == 1
    steps(resumed, [1, 2, 3])
    for which in range(4):
        if which != 1:
            assert same_bits(host(whole._array(which)), host(resumed._array(which))), which
    # the file is the reference's: torch.optim.Adam over 16 tensors of those shapes takes it
    ckpt = torch.load(path, weights_only=False)
    assert list(ckpt) == ["param_predictor", "optimizer"] and list(ckpt["param_predictor"]) == list(state0)
    free = [i for i, k in enumerate(state0) if k in T.FREE]
    assert free == [10, 11, 12, 13] and sorted(ckpt["optimizer"]["state"]) == [i for i in range(16) if i not in free]
    st = ckpt["optimizer"]["state"][0]["step"]
    assert st.dtype == torch.float32 and st.dim() == 0 and float(st) == 1.0
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(v.shape)) for v in state0.values()], lr=1e-4)
    opt.load_state_dict(ckpt["optimizer"])
    assert sorted(opt.state_dict()["state"]) == sorted(ckpt["optimizer"]["state"])
    # a checkpoint built from the real trainer's state after step 1, with and without entries for the gradient-free heads
    ends = []
    for with_free in (False, True):
        p = tmp_path / f"gold{int(with_free)}.pth"
        torch.save(golden_checkpoint(gold, state0, "a/after1", with_free), p)
        tr = trainer(state0)
        tr.load_model(p)
        steps(tr, [1, 2, 3])
        ends.append(host(tr.state_dict()))
        tr.close()
    assert same_bits(ends[0], ends[1])
    # the same state put in place without a file (the run that was never interrupted) ends on the same bits
    ck = golden_checkpoint(gold, state0, "a/after1", True)
    direct = trainer({k: v.numpy() for k, v in ck["param_predictor"].items()})
    direct._set(2, {k: ck["optimizer"]["state"][i]["exp_avg"] for i, k in enumerate(state0)})
    direct._set(3, {k: ck["optimizer"]["state"][i]["exp_avg_sq"] for i, k in enumerate(state0)})
    assert dev.lib.uwie_mlp_trainer_set_step_count(direct._handle, 1) == 0
    steps(direct, [1, 2, 3])
    assert same_bits(host(direct.state_dict()), ends[0])
    direct.close()
    e_par = max(float(np.abs(ends[0][k].astype(np.float64) - gold[f"a/after4/param/{k}"]).max()) for k in state0)
    assert e_par <= M * T.REF_TRAJ_ERROR[0]
    whole.close()
    resumed.close()


# ---------------------------------------------------------------- drawn masks
def test_drawn_masks(dev, big):
    import torch

    tr = trainer(big, seed=1234)
    rows = dev.tensor(np.random.default_rng(3).standard_normal((70, 79)))
    lib = dev.lib

    def draw(B, seed=1234):
        ws = dev.mlp_train_workspace(B, 256, 3)
        m = torch.full((7, B, 256), 9, dtype=torch.uint8, device=dev.torch_device)
        cols = dev.mlp_train_forward(tr._handle, rows[:B].contiguous(), ws, T.P_DROP, None, seed, m)
        return m.cpu().numpy(), cols, ws

    m70, cols, ws = draw(70)
    assert set(np.unique(m70)) == {0, 1}
    again, cols2, _ = draw(70)
    assert np.array_equal(m70, again) and np.array_equal(bits(cols), bits(cols2))  # the same (seed, step)
    m3, _, _ = draw(3)
    assert np.array_equal(m3, m70[:, :3])  # a bit depends on (seed, step, site, row, column), not on B
    other_seed, _, _ = draw(70, seed=1235)
    assert (other_seed != m70).mean() > 0.3
    assert lib.uwie_mlp_trainer_set_step_count(tr._handle, 1) == 0
    other_step, _, _ = draw(70)
    assert (other_step != m70).mean() > 0.3
    kept = float(m70.mean())
    print(f"kept {kept:.5f} of {m70.size}")
    assert m70.size == 70 * 256 * 7 and abs(kept - 0.7) <= 0.0065  # 5 sigma
    # the forward used these masks: given back, they give the same bits
    assert lib.uwie_mlp_trainer_set_step_count(tr._handle, 0) == 0
    given = dev.mlp_train_forward(tr._handle, rows, ws, T.P_DROP, dev_masks(dev, m70))
    assert np.array_equal(bits(given), bits(cols))
    tr.close()


def test_learning(dev, gold, state0):
    tr = trainer(state0, dropout=0.0, lr=1e-3)
    img, ref, feat = batch(dev, gold, 0)
    losses = [tr.train_step(img, ref, feat)[0] for _ in range(200)]
    print(f"loss {losses[0]:.6f} -> {losses[-1]:.6f}")
    assert losses[-1] < losses[0] and tr.step_count == 200
    tr.close()
