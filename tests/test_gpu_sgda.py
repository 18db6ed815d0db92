"""The SGDA learner on the GPU (include/fmhip_sgda.h): its update bit for bit against fmhip_step_compute + fmhip_step_apply where the
two coincide, one step — parameters, the sums S, the regularisers — against the fp64 twin of sgda_ref.py, the exact invariants
(run-to-run bits, group relabelling, a zero group, the clamp at +0, a zero packed gradient), the planted task end to end, and the
refusals on a live model.

Shapes: n + 1 in {37, 203} (no multiples of 4), 64 - 300 rows in 2 - 4 batches, k = 3 (packed rows, Kp = 32 with w in slot 3), 8 and 32
(k = Kp: no spare slot), and layout_cases' "page0" with its dense hot block.  A chunk of the plan holds 128 feature rows, so at
n + 1 = 203 one group spans two chunks."""
import ctypes as C

import numpy as np
import pytest

import layout_cases
import sgda_ref as sref
from test_gpu_parity import TOL_G

pytestmark = pytest.mark.gpu

ETA, REG0 = 0.05, 0.01
# max |S_gpu - S_twin| / sum|terms| over every case of test_one_step_vs_twin, measured on the MI355X (profiles/sgda.md): 2.2e-7.
# The bound is four times that; SURVEY section 8(c)'s per-element gradient tolerance, 1e-4, is its ceiling
S_MEASURED = 2.2e-7
S_BOUND = 4 * S_MEASURED
assert S_BOUND <= 1e-4


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def L():
    from sparkfm_amd import _ffi
    return _ffi.load()


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def problem(seed, n1, k, rows):
    """Rows of 1 - 8 distinct features below n1 - 1 with values in quarters, parameters at fp32 values."""
    rng = np.random.default_rng([seed, n1, k, rows])
    lens = rng.integers(1, 9, rows)
    rp = np.zeros(rows + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    col = np.concatenate([np.sort(rng.choice(n1 - 1, n, replace=False)) for n in lens]).astype(np.int32)
    val = rng.integers(1, 9, len(col)) / 4.0
    return dict(k=k, n1=n1, w0=0.125, w=f32(rng.normal(0, 0.1, n1)), v=f32(rng.normal(0, 0.1, (k, n1))), row_ptr=rp, col=col, val=val,
                y=f32(rng.normal(0, 1.0, rows)))


def labels(a, loss):
    return dict(a, y=(a["y"] > 0).astype(np.float64)) if loss == "logistic" else a


def groups_of(name, n1):
    i = np.arange(n1)
    table, G = {"one": (i * 0, 1), "fields2": ((i >= n1 // 3).astype(int), 2), "inter3": (i % 3, 3), "empty": ((i % 2) * 2, 3),
                "large": ((i >= 150).astype(int), 2)}[name]
    return np.ascontiguousarray(table, np.int32), G


SHAPES = {3: (37, 64, 32), 8: (203, 300, 75), 32: (203, 200, 100)}       # k -> n1, rows, batch_rows (2, 4 and 2 batches)


def model(fmhip, a, loss="squared"):
    """An FMModel at the problem's parameters, set to `loss`."""
    from sparkfm_amd import _ffi
    fm = fmhip.FMModel(a["n1"] - 1, a["k"])
    fm.w0, fm.w, fm.v = a["w0"], a["w"], a["v"]
    _ffi.check(L().fmhip_model_set_loss(fm.handle, _ffi.loss_code(loss)))
    return fm


def params(fm):
    return fm.w0, fm.w.copy(), fm.v.copy()


def same(x, y):
    return all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(x, y))


def new_handle(fm, table, G, lw, lv):
    from sparkfm_amd import _ffi
    h = C.c_void_p()
    _ffi.check(L().fmhip_sgda_create(fm.handle, _ffi.ptr(table), len(table), G, lw, lv, C.byref(h)))
    return h


def read_gradient(fm):
    """The packed gradient as the device holds it, through the experimental header's device read."""
    from sparkfm_amd import _ffi
    n, p = C.c_int64(), C.c_void_p()
    _ffi.check(L().fmhip_synchronize(fm.handle))
    _ffi.check(L().fmhip_grad_floats(fm.handle, C.byref(n)))
    _ffi.check(L().fmhip_grad_ptr(fm.handle, C.byref(p)))
    out = np.empty(n.value, np.float32)
    _ffi.check(L().fmhip_device_read(_ffi.ptr(out), p, out.nbytes, None))
    return out


# ---- 1. bit parity with the existing step -------------------------------------------------------------------------------------

def parity(fmhip, a, build, loss, G):
    """Five fmhip_sgda_steps without validation at lambda_w = regw, lambda_v = regv == five fmhip_step_compute + fmhip_step_apply."""
    from sparkfm_amd import _ffi
    regw, regv = 0.02, 0.03
    outs = []
    for sgda in (True, False):
        ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], **build).cache()
        fm = model(fmhip, a, loss)
        h = new_handle(fm, np.ascontiguousarray(np.arange(a["n1"]) % G, np.int32), G, regw, regv) if sgda else None
        for t in range(5):
            b = t % ds.n_batches
            if sgda:
                _ffi.check(L().fmhip_sgda_step(h, ds.handle, b, None, 0, ETA, 0.0, REG0, None, None))
            else:
                _ffi.check(L().fmhip_step_compute(fm.handle, ds.handle, b))
                _ffi.check(L().fmhip_step_apply(fm.handle, ETA, REG0, regw, regv))
        fm._device_updated()
        outs.append(params(fm))
        if sgda:
            assert not read_gradient(fm)[32:].any()          # the rows are zero, as fmhip_step_apply leaves them
            _ffi.check(L().fmhip_sgda_destroy(h))
        ds.unpersist()
        fm.close()
    assert not same(outs[0], (a["w0"], a["w"], a["v"]))      # something was trained
    assert same(outs[0], outs[1])


@pytest.mark.parametrize("G", [1, 3])
@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k", [3, 8, 32])
def test_update_is_the_existing_step_bit_for_bit(fmhip, k, loss, G):
    n1, rows, br = SHAPES[k]
    parity(fmhip, labels(problem(11, n1, k, rows), loss), dict(batch_rows=br), loss, G)


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_update_is_the_existing_step_on_a_hot_block_layout(fmhip, loss):
    lay = layout_cases.layout("page0", 8, loss)
    ds = fmhip.DataSet(lay.a["row_ptr"], lay.a["col"], lay.a["val"], lay.a["y"], **lay.build).cache()
    assert sorted(i for i in ds.layout()["hot_ids_all"] if i >= 0) == lay.hot_ids_all and lay.hot_pages >= 1
    ds.unpersist()
    parity(fmhip, dict(lay.a, w=f32(lay.a["w"]), v=f32(lay.a["v"])), lay.build, loss, 3)


# ---- 2. one step against the twin ------------------------------------------------------------------------------------------------

def one_step(fmhip, a, av, build, vbuild, group, G, loss, batch, vbatch, lam=(0.05, 0.08), eta_lambda=0.5):
    """-> (the learner with its handle, fm, the twin's state before and after, the twin's step record)."""
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], **build).cache()
    val = fmhip.DataSet(av["row_ptr"], av["col"], av["val"], av["y"], **vbuild).cache()
    fm = model(fmhip, a, loss)
    sgda = fmhip.HipSGDA(validation=val, groups=group, eta=ETA, eta_lambda=eta_lambda, reg0=REG0, loss=loss)
    assert sgda.n_groups == G
    sgda._handle(fm)
    lw = f32(np.full(G, lam[0]) * (1 + 0.1 * np.arange(G)))
    lv = f32(np.full((a["k"], G), lam[1]) * (1 + 0.05 * np.arange(a["k"]))[:, None])
    sgda.set_state(lw, lv)
    st = sgda.step(fm, ds, batch, vbatch)
    X, Xv = sref.dense(a["row_ptr"], a["col"], a["val"], a["n1"]), sref.dense(av["row_ptr"], av["col"], av["val"], a["n1"])
    r0, r1 = batch * build["batch_rows"], min(len(a["y"]), (batch + 1) * build["batch_rows"])
    c0, c1 = vbatch * vbuild["batch_rows"], min(len(av["y"]), (vbatch + 1) * vbuild["batch_rows"])
    s0 = sref.State(a["w0"], a["w"], a["v"], G, lw, lv)
    s1 = s0.copy()
    rec = sref.step(s1, group, X[r0:r1], a["y"][r0:r1], Xv[c0:c1], av["y"][c0:c1], ETA, eta_lambda, REG0, loss)
    assert st[0]["rows"] == r1 - r0 and st[1]["rows"] == c1 - c0
    assert st[0]["sse"] == pytest.approx(float((rec["e_train"] ** 2).sum()), rel=1e-5)
    assert st[1]["sse"] == pytest.approx(float((rec["e_val"] ** 2).sum()), rel=1e-5)
    return sgda, fm, (ds, val), s0, s1, rec


def check_one_step(sgda, fm, s0, s1, rec, eta_lambda=0.5):
    """theta': per feature row, the step's change is held to eta times test_gpu_parity's gradient tolerance — TOL_G of the row's
    largest gradient entry, floored at 1e-3 of the largest of all — plus the fp32 rounding of the stored value.  S: S_BOUND of the sum
    of the terms' magnitudes.  lambda follows from S by one fma and a clamp (1-Lipschitz): the same bound times the rate, plus its
    own fp32 rounding."""
    gv, gw = (s0.v - s1.v) / ETA, (s0.w - s1.w) / ETA
    scale = max(np.abs(gv).max(), np.abs(gw).max(), 1e-6)
    tol_v = ETA * TOL_G * np.maximum(np.abs(gv).max(axis=0), 1e-3 * scale)[None, :] + 1.2e-7 * np.abs(s1.v)
    tol_w = ETA * TOL_G * np.maximum(np.abs(gw), 1e-3 * scale) + 1.2e-7 * np.abs(s1.w)
    assert (np.abs(fm.v - s1.v) <= tol_v).all(), float((np.abs(fm.v - s1.v) / tol_v).max())
    assert (np.abs(fm.w - s1.w) <= tol_w).all(), float((np.abs(fm.w - s1.w) / tol_w).max())
    assert abs(fm.w0 - s1.w0) <= ETA * TOL_G * max(abs(s0.w0 - s1.w0) / ETA, 1e-3) + 1.2e-7 * abs(s1.w0)
    sw, sv = sgda.last_sums()
    # (a group without a term has S = 0 on both sides: the ratio's denominator is floored far below any term)
    ratio = max(float((np.abs(sw - rec["S_w"]) / np.maximum(rec["T_w"], 1e-30)).max()), float((np.abs(sv - rec["S_v"]) / np.maximum(rec["T_v"], 1e-30)).max()))
    print("SGDA_S_RATIO %.4g" % ratio)
    assert ratio <= S_BOUND, ratio
    st = sgda.state
    rate = eta_lambda * ETA
    assert (np.abs(st["lambda_w"] - s1.lw) <= rate * S_BOUND * rec["T_w"] + 1.2e-7 * s1.lw).all()
    assert (np.abs(st["lambda_v"] - s1.lv) <= rate * S_BOUND * rec["T_v"] + 1.2e-7 * s1.lv).all()
    assert (st["lambda_w"] >= 0).all() and (st["lambda_v"] >= 0).all() and st["steps"] == 1
    assert not (st["lambda_w"] == f32(s0.lw)).all()             # the step moved them


def finish(sgda, fm, sets):
    sgda.close()
    for d in sets:
        d.unpersist()
    fm.close()


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k,name", [(3, "one"), (3, "inter3"), (8, "fields2"), (8, "inter3"), (8, "empty"), (8, "large"), (32, "one"), (32, "inter3")])
def test_one_step_vs_twin(fmhip, k, name, loss):
    n1, rows, br = SHAPES[k]
    a, av = labels(problem(21, n1, k, rows), loss), labels(problem(22, n1, k, 96), loss)
    group, G = groups_of(name, n1)
    sgda, fm, sets, s0, s1, rec = one_step(fmhip, a, av, dict(batch_rows=br), dict(batch_rows=48), group, G, loss, 1, 1)
    if name == "empty":
        assert sgda.group_counts.tolist() == np.bincount(group, minlength=3).tolist() and sgda.group_counts[1] == 0
        assert sgda.last_sums()[0][1] == 0 and (sgda.last_sums()[1][:, 1] == 0).all()
    if name in ("one", "large"):
        assert sgda.group_counts.max() > 128 or n1 < 128        # n1 = 203: a group larger than a chunk
    check_one_step(sgda, fm, s0, s1, rec)
    assert not read_gradient(fm).any()                          # the whole packed gradient, head included
    finish(sgda, fm, sets)


@pytest.mark.parametrize("name", ["one", "large"])
def test_one_step_vs_twin_with_many_chunks(fmhip, name):
    """n + 1 = 2203: a group of 18 chunks (one) and one of 17 beside one of 2 (large) — k_sgda_lambda_step adds a group's partials
    sixteen loads at a time and the rest one by one; both loops run here, and at the other shapes only the second."""
    a, av = problem(23, 2203, 3, 64), problem(24, 2203, 3, 96)
    group, G = groups_of(name, 2203)
    sgda, fm, sets, s0, s1, rec = one_step(fmhip, a, av, dict(batch_rows=32), dict(batch_rows=48), group, G, "squared", 1, 0)
    assert -(-int(sgda.group_counts.max()) // 128) in (17, 18)
    check_one_step(sgda, fm, s0, s1, rec)
    assert not read_gradient(fm).any()
    finish(sgda, fm, sets)


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_one_step_vs_twin_on_a_hot_block_layout(fmhip, loss):
    """layout_cases' page0 (1200 x 500, twelve features in the dense hot block, batches of 297 rows) as the train AND the validation
    set: the validation gradient of the hot features comes from the block product."""
    lay = layout_cases.layout("page0", 8, loss)
    a = dict(lay.a, w=f32(lay.a["w"]), v=f32(lay.a["v"]), y=f32(lay.a["y"]))
    group, G = groups_of("inter3", a["n1"])
    sgda, fm, sets, s0, s1, rec = one_step(fmhip, a, a, lay.build, lay.build, group, G, loss, 0, 1)
    assert sorted(i for i in sets[1].layout()["hot_ids_all"] if i >= 0) == lay.hot_ids_all
    check_one_step(sgda, fm, s0, s1, rec)
    assert not read_gradient(fm).any()
    finish(sgda, fm, sets)


# ---- 3. exact invariants ---------------------------------------------------------------------------------------------------------

def three_epochs(fmhip, a, av, group, G, k, shuffle_seed=5):
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=75).cache()
    val = fmhip.DataSet(av["row_ptr"], av["col"], av["val"], av["y"], batch_rows=48).cache()
    fm = model(fmhip, a)
    sgda = fmhip.HipSGDA(validation=val, groups=group, eta=ETA, eta_lambda=0.5, init_lambda=0.02, shuffle_seed=shuffle_seed)
    assert sgda.n_groups == G
    for _ in range(3):
        sgda.learn(fm, ds)
    out = params(fm), sgda.state, sgda.last_validation_stats
    finish(sgda, fm, (ds, val))
    return out


def test_runs_repeat_and_relabelling_permutes_lambda(fmhip):
    """Two runs of three epochs give the same bits; relabelling the groups by a permutation permutes lambda's columns bit for bit and
    leaves the parameters' bits alone."""
    a, av = problem(31, 203, 8, 300), problem(32, 203, 8, 96)
    group, G = groups_of("inter3", 203)
    p1, s1, v1 = three_epochs(fmhip, a, av, group, G, 8)
    p2, s2, v2 = three_epochs(fmhip, a, av, group, G, 8)
    assert same(p1, p2) and np.array_equal(s1["lambda_w"], s2["lambda_w"]) and np.array_equal(s1["lambda_v"], s2["lambda_v"])
    assert s1["steps"] == 12 and v1 == v2 and v1["rows"] == 4 * 48 and v1["steps"] == 4      # (the last epoch's four validation batches)
    assert len(set(s1["lambda_w"].tolist())) == 3               # the groups did part ways
    perm = np.array([2, 0, 1], np.int32)                        # old group a is now perm[a]
    p3, s3, _ = three_epochs(fmhip, a, av, perm[group], G, 8)
    assert same(p1, p3)
    assert np.array_equal(s3["lambda_w"][perm], s1["lambda_w"]) and np.array_equal(s3["lambda_v"][:, perm], s1["lambda_v"])


@pytest.mark.parametrize("k", [3, 8])
def test_a_zero_group_has_zero_sums_and_keeps_its_lambda(fmhip, k):
    n1, rows, br = SHAPES[k]
    a, av = problem(41, n1, k, rows), problem(42, n1, k, 96)
    group, G = groups_of("inter3", n1)
    a["w"][group == 1] = 0.0
    a["v"][:, group == 1] = 0.0
    sgda, fm, sets, s0, s1, rec = one_step(fmhip, a, av, dict(batch_rows=br), dict(batch_rows=48), group, G, "squared", 0, 0)
    sw, sv = sgda.last_sums()
    assert sw[1] == 0 and (sv[:, 1] == 0).all() and sw[0] != 0 and (sv[:, 0] != 0).all()
    st = sgda.state
    assert st["lambda_w"][1] == f32(s0.lw)[1] and np.array_equal(st["lambda_v"][:, 1], f32(s0.lv)[:, 1])
    assert st["lambda_w"][0] != f32(s0.lw)[0]
    assert (fm.v[:, group == 1] != 0).any()                     # the group's parameters did take their train step
    finish(sgda, fm, sets)


@pytest.mark.parametrize("k", [3, 32])
def test_the_clamp_leaves_exactly_plus_zero(fmhip, k):
    """eta_lambda = 1e4: wherever S < 0 the step would go far below zero — lambda is +0 there, bit for bit, and nowhere negative."""
    n1, rows, br = SHAPES[k]
    a, av = problem(51, n1, k, rows), problem(52, n1, k, 96)
    group, G = groups_of("inter3", n1)
    sgda, fm, sets, s0, s1, rec = one_step(fmhip, a, av, dict(batch_rows=br), dict(batch_rows=48), group, G, "squared", 0, 0, eta_lambda=1e4)
    st = sgda.state
    rate = 1e4 * ETA
    pre_w, pre_v = s0.lw + rate * rec["S_w"], s0.lv + rate * rec["S_v"]          # the twin's lambda before the clamp
    assert (pre_w < -1e-3).any() or (pre_v < -1e-3).any()
    assert (pre_w > 1e-3).any() or (pre_v > 1e-3).any()
    for lam, pre in ((st["lambda_w"], pre_w), (st["lambda_v"], pre_v)):
        assert (lam[pre < -1e-3] == 0).all() and (lam[pre > 1e-3] > 0).all() and not np.signbit(lam).any() and (lam >= 0).all()
    finish(sgda, fm, sets)


# ---- 4. end to end: the planted task ------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def twin_runs():
    """The twin's 150 epochs, once per (seed, loss)."""
    out = {}
    for loss in ("squared", "logistic"):
        for seed in sref.SEEDS:
            t = sref.planted(seed, loss)
            s, val, test = sref.run_planted(t, t["group"], 2, sref.ETA_LAMBDA, loss=loss)
            fixed = None
            if loss == "squared":
                fixed = [sref.run_planted(t, np.zeros(t["n1"], np.int32), 1, 0.0, lam, validation=False)[2] for lam in sref.FIXED]
            out[seed, loss] = dict(task=t, state=s, val=val, test=test, fixed=fixed)
    return out


def planted_sets(fmhip, t):
    sets = []
    for name in ("train", "val", "test"):
        X, y = t[name]
        rp, col, v = sref.csr(X)
        sets.append(fmhip.DataSet(rp, col, v, y, batch_rows=sref.BATCH if name != "test" else 0).cache())
    return sets


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("seed", sref.SEEDS)
def test_planted_task_end_to_end(fmhip, twin_runs, seed, loss):
    """150 epochs of HipSGDA, two groups: the final validation and test loss match the twin within 1e-5 (test_gpu_ftrl.py's tolerance for
    a trained loss); squared: the host test's orderings hold on the device — below the best fixed lambda of the grid, the noise
    group's lambda_w above the informative group's, no lambda negative."""
    r = twin_runs[seed, loss]
    t = r["task"]
    train, val, test = planted_sets(fmhip, t)
    fm = fmhip.FMModel(t["n1"] - 1, t["k"])
    fm.w0, fm.w, fm.v = t["w0"], t["w"], t["v"]
    sgda = fmhip.HipSGDA.run(validation=val, groups=t["group"], eta=sref.ETA, eta_lambda=sref.ETA_LAMBDA, loss=loss)
    for _ in range(sref.EPOCHS):
        sgda.learn(fm, train)
    st, vs = sgda.state, sgda.last_validation_stats
    got_test = fm.computeRMSE(test) if loss == "squared" else fm.computeLogLoss(test)
    print("seed %d %s: validation %.6f (twin %.6f), test %.6f (twin %.6f), lambda_w %s (twin %s)" % (
        seed, loss, vs["rmse"], r["val"], got_test, r["test"], st["lambda_w"].tolist(), r["state"].lw.tolist()))
    assert st["steps"] == sref.EPOCHS * 8 and vs["rows"] == 8 * sref.BATCH
    assert vs["rmse"] == pytest.approx(r["val"], rel=1e-5)
    assert got_test == pytest.approx(r["test"], rel=1e-5)
    if loss == "logistic":
        Xv, yv = t["val"]
        s = r["state"]
        assert vs["logloss"] == pytest.approx(sref.logloss(sref.predict(s.w0, s.w, s.v, Xv)[0], yv), rel=1e-5)
    else:
        assert got_test < min(r["fixed"])
        assert st["lambda_w"][1] > st["lambda_w"][0]
    assert (st["lambda_w"] >= 0).all() and (st["lambda_v"] >= 0).all()
    finish(sgda, fm, (train, val, test))


def test_fixed_per_group_regularisation(fmhip):
    """validation=None, eta_lambda=0, a (lambda_w, lambda_v) pair: per-group-regularised SGD — three epochs track the twin, the
    regularisers never move, and each group decays at its own rate."""
    a = problem(61, 203, 8, 300)
    group, G = groups_of("fields2", 203)
    lw, lv = np.array([0.0, 0.25]), np.array([[0.0, 0.5]] * 8)
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=75).cache()
    fm = model(fmhip, a)
    sgda = fmhip.HipSGDA.run(groups=group, eta=ETA, eta_lambda=0, init_lambda=(lw, lv), reg0=REG0)
    s = sref.State(a["w0"], a["w"], a["v"], G, lw, lv)
    X = sref.dense(a["row_ptr"], a["col"], a["val"], 203)
    for _ in range(3):
        sgda.learn(fm, ds)
        sse = sref.epoch(s, group, X, a["y"], None, None, 75, ETA, 0.0, REG0)[0]
        assert sgda.last_stats["sse"] == pytest.approx(sse, rel=1e-5)
    assert sgda.last_validation_stats is None and sgda.state["steps"] == 12
    assert np.array_equal(sgda.state["lambda_w"], lw) and np.array_equal(sgda.state["lambda_v"], lv)
    # (test_gpu_parity.test_sgd_epochs_track_the_oracle's tolerance for trained parameters)
    assert np.linalg.norm(fm.v - s.v) <= 1e-4 * np.linalg.norm(s.v) and np.linalg.norm(fm.w - s.w) <= 1e-4 * np.linalg.norm(s.w)
    untouched = np.setdiff1d(np.arange(203), a["col"])
    assert len(untouched) and (group[untouched] == 1).any()
    u1 = untouched[group[untouched] == 1]
    np.testing.assert_allclose(fm.v[:, u1], a["v"][:, u1] * (1 - ETA * 0.5) ** 12, rtol=2e-6)      # twelve steps of its group's decay
    finish(sgda, fm, (ds,))


# ---- 5. refusals on a live model -------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_model_alone(fmhip):
    from sparkfm_amd import _ffi
    a = problem(71, 37, 3, 64)
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=32).cache()
    fm = model(fmhip, a)
    table = np.zeros(37, np.int32)
    before = params(fm)
    h = C.c_void_p()
    err = L().fmhip_last_error

    def create(tab=table, n=37, G=1):
        return L().fmhip_sgda_create(fm.handle, _ffi.ptr(tab), n, G, 0.0, 0.0, C.byref(h))
    # the table against the model
    assert create(n=36) == -1 and b"num_attribute + 1 = 37" in err()
    bad = table.copy()
    bad[17] = 2
    assert create(tab=bad, G=2) == -1 and b"feature 17 has group id 2" in err()
    bad[17] = -1
    assert create(tab=bad, G=2) == -1 and b"feature 17" in err()
    # the model's rule, at create
    _ffi.check(L().fmhip_model_set_optimizer(fm.handle, _ffi.OPT_ADAGRAD, 1e-10, 0.1))
    assert create() == -5 and b"AdaGrad" in err()
    _ffi.check(L().fmhip_model_set_ftrl(fm.handle, 1.0, 0.1, 0.0, 0.0))
    assert create() == -5 and b"FTRL" in err()
    _ffi.check(L().fmhip_model_set_optimizer(fm.handle, _ffi.OPT_SGD, 1e-10, 0.1))
    _ffi.check(L().fmhip_model_set_pairing(fm.handle, _ffi.PAIRING_ADJACENT))
    assert create() == -5 and b"pairs" in err()
    _ffi.check(L().fmhip_model_set_pairing(fm.handle, _ffi.PAIRING_NONE))
    assert h.value is None
    # ... and at a step of a handle made while the model was plain SGD
    assert create() == 0

    def step(train=ds, val=None, eta_lambda=0.0, b=0, vb=0):
        return L().fmhip_sgda_step(h, train.handle, b, None if val is None else val.handle, vb, ETA, eta_lambda, 0.0, None, None)
    _ffi.check(L().fmhip_model_set_optimizer(fm.handle, _ffi.OPT_ADAGRAD, 1e-10, 0.1))
    assert step() == -5 and b"AdaGrad" in err()
    _ffi.check(L().fmhip_model_set_ftrl(fm.handle, 1.0, 0.1, 0.0, 0.0))
    assert step() == -5 and b"FTRL" in err()
    _ffi.check(L().fmhip_model_set_optimizer(fm.handle, _ffi.OPT_SGD, 1e-10, 0.1))
    _ffi.check(L().fmhip_model_set_pairing(fm.handle, _ffi.PAIRING_ADJACENT))
    assert step() == -5 and b"pairs" in err()
    _ffi.check(L().fmhip_model_set_pairing(fm.handle, _ffi.PAIRING_NONE))
    # the datasets
    weighted = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=32, weights=np.ones(64)).cache()
    scoring = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], scoring=True).cache()
    assert step(train=weighted) == -5 and b"example weights" in err()
    assert step(val=weighted, eta_lambda=0.1) == -5 and b"example weights" in err()
    assert step(val=scoring, eta_lambda=0.1) == -1 and b"fmhip_rows_create" in err()
    assert step(train=scoring) == -5 and b"scoring only" in err()          # (a train set without transposes: fmhip_sgd_step's own refusal)
    assert step(eta_lambda=0.1) == -1 and b"needs a validation set" in err()
    assert step(b=2) == -1 and step(val=ds, vb=2) == -1 and step(b=-1) == -1
    assert L().fmhip_sgda_epoch(h, ds.handle, None, ETA, 0.1, 0.0, None, None, None) == -1 and b"needs a validation set" in err()
    order = np.array([0, 2], np.int64)
    assert L().fmhip_sgda_epoch(h, ds.handle, None, ETA, 0.0, 0.0, _ffi.ptr(order), None, None) == -1
    # lambda's setter
    lw, lv = np.array([0.1]), np.full((3, 1), 0.2)
    for bad_w, bad_v in ((np.array([-0.1]), lv), (lw, np.array([[0.2], [np.nan], [0.2]])), (np.array([np.inf]), lv)):
        assert L().fmhip_sgda_set_lambda(h, _ffi.ptr(bad_w), _ffi.ptr(np.ascontiguousarray(bad_v))) == -1 and b"finite and >= 0" in err()
    assert L().fmhip_sgda_set_lambda(h, None, _ffi.ptr(lv)) == -1
    got_w, got_v = np.empty(1), np.empty((3, 1))
    _ffi.check(L().fmhip_sgda_get_lambda(h, _ffi.ptr(got_w), _ffi.ptr(got_v)))
    assert got_w[0] == 0 and not got_v.any()                       # every refusal left the handle as it was
    steps = C.c_int64(-1)
    _ffi.check(L().fmhip_sgda_info(h, None, None, C.byref(steps)))
    assert steps.value == 0
    # relational data, through the learner
    rd = fmhip.RelationalData([1.0], [fmhip.Relation([([0], [1.0])], [0])])
    with pytest.raises(_ffi.FmhipError) as e:
        fmhip.HipSGDA.run(eta_lambda=0).learn(fm, rd)
    assert e.value.code == -5
    fm._device_updated()                                           # (read the device's copy again)
    assert same(params(fm), before)                                # not a bit of the model moved
    assert not read_gradient(fm).any()
    # and the handle still works
    assert step() == 0
    fm._device_updated()
    assert not same(params(fm), before)
    _ffi.check(L().fmhip_sgda_destroy(h))
    for d in (ds, weighted, scoring):
        d.unpersist()
    fm.close()
