"""Binary classification: the logistic loss on every training path, and log-loss scoring (fmhip_model_set_loss, fmhip_logloss).

The fp64 reference is train_ref.py's: the unchanged squared-loss oracle at the pseudo-targets y' = yhat - (sigmoid(yhat) - [y > 0]).
Tolerances as in test_gpu_parity.py (TOL_Y, TOL_G, check_grad) and test_gpu_world8.py (rel-L2 1e-5 for the data-parallel runs)."""
import ctypes as C

import numpy as np
import pytest

import oracle
from helpers import random_problem
from test_gpu_parity import check_grad
from train_ref import DP_FRACTIONS, DP_ROWS, Rule, State, dp_epochs, dp_init, dp_shard, epochs, make, pseudo_targets, rel, sigmoid

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def L():
    from sparkfm_amd import _ffi
    return _ffi.load()


def set_loss(fm, loss):
    from sparkfm_amd import _ffi
    _ffi.check(L().fmhip_model_set_loss(fm.handle, _ffi.loss_code(loss)))


def logloss_np(yh, y):
    t = (np.asarray(y) > 0).astype(np.float64)
    return np.maximum(yh, 0.0) - t * yh + np.log1p(np.exp(-np.abs(yh)))


def binary_problem(seed, n_rows, n1, k, lo, hi, empty_rows=(), labels01=True):
    a = random_problem(seed, n_rows, n1, k, lo, hi, empty_rows=empty_rows)
    t = np.random.default_rng(seed + 1).random(n_rows) < 0.4
    a["y"] = np.where(t, 1.0, 0.0 if labels01 else -1.0)
    return a


def check_batches(fm, ds, a, batch_rows):
    """Every batch's logistic gradient (fmhip_batch_grad) against the pseudo-target oracle."""
    n = len(a["y"])
    yp, e, _ = pseudo_targets(a["w0"], a["w"], a["v"], a["row_ptr"], a["col"], a["val"], a["y"], "logistic")
    for b in range(ds.n_batches):
        r0, r1 = b * batch_rows, min(n, (b + 1) * batch_rows)
        gv, gw, g0, st = fm.batchGradient(ds, b)
        ogv, ogw, og0, osse, oe = oracle.batch_grad(a["w0"], a["w"], a["v"], r0, r1, a["row_ptr"], a["col"], a["val"], yp)
        np.testing.assert_allclose(oe, e[r0:r1], rtol=1e-12, atol=1e-12)       # the oracle's residual at y' IS the logistic one
        check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
        assert g0 == pytest.approx(og0, rel=1e-5, abs=1e-4)
        assert st["sum_e"] == pytest.approx(e[r0:r1].sum(), rel=1e-5, abs=1e-4)
        assert st["sse"] == pytest.approx(osse, rel=1e-5)
        assert st["rows"] == r1 - r0 and st["nonfinite"] == 0


@pytest.mark.parametrize("k", [4, 31, 32, 64, 129, 256])
def test_logistic_gradient_vs_pseudo_target_oracle(fmhip, k):
    """fmhip_batch_grad under the logistic loss, labels {0,1}: a packed slot (k < Kp), k = Kp (e in the P row's low bits), the
    J = 2 / 4 geometries; empty rows, ragged last batch."""
    a = binary_problem(500 + k, 1000, 257, k, 0, 40, empty_rows=(0, 17, 999))
    ds, fm = make(fmhip, a, batch_rows=300)
    set_loss(fm, "logistic")
    check_batches(fm, ds, a, 300)
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("k", [16, 32, 64])
def test_logistic_gradient_with_hot_pages(fmhip, k):
    """The same with the dense hot block (forward prologue + the MFMA block product of the gradient): features 0..39 sit in
    10-40 % of the rows."""
    from sparkfm_amd import _ffi
    a = binary_problem(900 + k, 1200, 400, k, 3, 30, empty_rows=(5,))
    rng = np.random.default_rng(k)
    rp, cols, vals = [0], [], []
    for r in range(1200):
        s = slice(a["row_ptr"][r], a["row_ptr"][r + 1])
        c, x = a["col"][s], a["val"][s]
        if r != 5:
            hot = np.flatnonzero(rng.random(40) < np.linspace(0.4, 0.1, 40))
            keep = ~np.isin(c, hot)
            c = np.concatenate([c[keep], hot.astype(np.int32)])
            x = np.concatenate([x[keep], rng.uniform(0.2, 1.0, len(hot))])
        cols.append(c)
        vals.append(x)
        rp.append(rp[-1] + len(c))
    a.update(row_ptr=np.array(rp, np.int64), col=np.concatenate(cols).astype(np.int32), val=np.concatenate(vals))
    try:
        L().fmhip_tune(_ffi.TUNE_HOT_BLOCK, 1)
        ds, fm = make(fmhip, a, batch_rows=500)
    finally:
        L().fmhip_tune(_ffi.TUNE_HOT_BLOCK, 1)
    assert len(ds.layout()["hot_ids"]) == 16                # the case is what it claims: a full two-sided page
    set_loss(fm, "logistic")
    check_batches(fm, ds, a, 500)
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("case", ["no_decay", "wide_lazy_decay"])
def test_logistic_sgd_trajectory(fmhip, case):
    """Two shuffled epochs of fmhip_sgd_epoch (HipSGD(loss="logistic")) against the stepped pseudo-target oracle.  The wide case
    (n+1 = 20000, a batch touches a few hundred rows, regv > 0) takes the rows-only update with lazy decay."""
    if case == "no_decay":
        a = binary_problem(31, 1200, 300, 32, 2, 30, empty_rows=(7,))
        regs, br = (0.0, 0.0, 0.0), 300
    else:
        a = binary_problem(32, 800, 20000, 64, 2, 10)
        regs, br = (1e-3, 1e-3, 2e-3), 100
    ds, fm = make(fmhip, a, batch_rows=br)
    sgd = fmhip.HipSGD(eta=0.1, reg0=regs[0], regw=regs[1], regv=regs[2], shuffle_seed=11, loss="logistic")
    orders = []
    for _ in range(2):
        orders.append(sgd.batch_order(ds.n_batches).tolist())
        sgd.learn(fm, ds)
    assert sgd.last_stats["rows"] == len(a["y"])
    ow0, ow, ov = epochs(State(a["w0"], a["w"], a["v"]), a, br, orders, 0.1, *regs, Rule("logistic")).params()
    assert rel(fm.v, ov) <= 1e-4 and rel(fm.w, ow) <= 1e-4, (rel(fm.v, ov), rel(fm.w, ow))
    assert fm.w0 == pytest.approx(ow0, rel=1e-4, abs=1e-6)
    assert np.abs(fm.w - a["w"]).max() > 1e-3                # it moved
    ds.unpersist()
    fm.close()


# ---- data-parallel: thread ranks over ThreadStagedComm (every collective staged through the host) ----

@pytest.mark.parametrize("world,exchange,reverse_ids", [(w, x, False) for w in (2, 8) for x in ("dense", "sharded", "touched", "pipelined")]
                         + [(2, "pipelined", True)])
def test_logistic_data_parallel(fmhip, world, exchange, reverse_ids):
    """HipDataParallelSGD(loss="logistic") with `world` thread ranks: replicas bit-identical, the pseudo-target oracle over the
    global batches matched.  The pipelined exchange finishes rows in pass B; reverse_ids puts the dense hot block's features at
    or above the top cut, so pass B also runs the hot prologue."""
    from sparkfm_amd import DataSet, FMModel
    from sparkfm_amd.distributed import HipDataParallelSGD, ThreadStagedComm, run_thread_ranks
    rows, n1_data, n1, k, br, n_epochs = DP_ROWS[world], 800, 803, 32, 250, 2
    eta, regw, regv = 0.1, 1e-3, 1e-3
    shards = [dp_shard(4321, rows[r], r, rows, n1_data, reverse_ids, binary=True) for r in range(world)]

    def rank_fn(r, group):
        ds = DataSet.from_arrays(shards[r], batch_rows=br, device=0).cache()
        fm = FMModel(n1 - 1, k, device=0)
        fm.w0, fm.w, fm.v = dp_init(n1, k)
        comm = ThreadStagedComm(fm, r, group)
        dp = HipDataParallelSGD(comm, eta=eta, regw=regw, regv=regv, exchange=exchange, upper_fractions=DP_FRACTIONS[exchange],
                                loss="logistic")
        dp.plan(fm, ds)
        hot_top = reverse_ids and max(ds.layout()["hot_ids"]) >= max(dp.cuts)
        for _ in range(n_epochs):
            dp.learn(fm, ds)
        out = dict(w0=fm.w0, w=fm.w.copy(), v=fm.v.copy(), hot_top=hot_top)
        group.barrier()
        comm.close()
        ds.unpersist()
        fm.close(discard=True)
        return out

    res = run_thread_ranks(world, rank_fn, timeout=300.0)
    for r in range(1, world):
        assert np.array_equal(res[0]["v"], res[r]["v"]) and np.array_equal(res[0]["w"], res[r]["w"]) and res[0]["w0"] == res[r]["w0"], r
    if reverse_ids:
        assert res[0]["hot_top"]
    ow0, ow, ov = dp_epochs(State(*dp_init(n1, k)), shards, br, [None] * n_epochs, eta, 0.0, regw, regv, Rule("logistic")).params()
    assert rel(res[0]["v"], ov) <= 1e-5 and rel(res[0]["w"], ow) <= 1e-5, (rel(res[0]["v"], ov), rel(res[0]["w"], ow))
    assert abs(res[0]["w0"] - ow0) <= 1e-5 * abs(ow0) + 1e-6


@pytest.mark.parametrize("world", [2, 8])
def test_data_parallel_plan_refuses_mixed_losses(fmhip, world):
    """Ranks whose models train under different losses: fmhip_dp_plan fails on EVERY rank (the loss and its complement travel
    in the plan's max-reduce), nobody is left inside a collective.  A loss changed after the plan is this rank's own failure:
    it contributes zeros and reports the error, the peers step on."""
    from sparkfm_amd import DataSet, FMModel, _ffi
    from sparkfm_amd.distributed import HipDataParallelSGD, ThreadStagedComm, run_thread_ranks
    rows = DP_ROWS[world]
    shards = [dp_shard(99, rows[r], r, rows, 300, binary=True) for r in range(world)]

    def rank_fn(r, group):
        ds = DataSet.from_arrays(shards[r], batch_rows=250, device=0).cache()
        fm = FMModel(302, 16, device=0)
        fm.w0, fm.w, fm.v = dp_init(303, 16)
        comm = ThreadStagedComm(fm, r, group)
        dp = HipDataParallelSGD(comm, eta=0.1, exchange="dense", upper_fractions=(0.3,), loss="logistic" if r == 1 else "squared")
        out = {}
        try:
            dp.plan(fm, ds)
            out["plan"] = 0
        except _ffi.FmhipError as ex:
            out["plan"] = ex.code
        # the same losses everywhere: the plan passes; then rank 1 switches its loss behind the plan's back
        dp2 = HipDataParallelSGD(comm, eta=0.1, exchange="dense", upper_fractions=(0.3,), loss="squared")
        dp2.plan(fm, ds)
        if r == 1:
            _ffi.check(L().fmhip_model_set_loss(fm.handle, _ffi.LOSS_LOGISTIC))
        st = _ffi.Stats()
        out["epoch"] = L().fmhip_dp_epoch(fm.handle, ds.handle, comm.handle, 0.1, 0.0, 0.0, 0.0, C.byref(st))
        group.barrier()
        comm.close()
        ds.unpersist()
        fm.close(discard=True)
        return out

    res = run_thread_ranks(world, rank_fn, timeout=120.0)
    assert [o["plan"] for o in res] == [-1] * world
    # dp_epoch agrees local_checks over all ranks first: every rank stops before its first collective
    assert [o["epoch"] for o in res] == [-1] * world


def test_logloss_vs_numpy(fmhip):
    """fmhip_logloss: mean log-loss rel 1e-5 against numpy fp64 on the oracle's margins; the Brier sum and sum_e over
    sigmoid(yhat) - t.  Saturated margins (w0 = +-40) stay finite and accurate; an infinite weight is counted in nonfinite (the
    margin is not finite though sigmoid(inf) is) and the mean is not finite."""
    a = binary_problem(61, 1500, 300, 24, 0, 30, empty_rows=(3,), labels01=False)       # labels {-1, +1}
    ds, fm = make(fmhip, a, batch_rows=500)
    for w0 in (a["w0"], 40.0, -40.0):
        fm.w0 = w0
        r, st = C.c_double(), _ffi_stats()
        assert L().fmhip_logloss(fm.handle, ds.handle, C.byref(r), C.byref(st)) == 0
        yh = oracle.predict(w0, a["w"], a["v"], a["row_ptr"], a["col"], a["val"])
        ll = logloss_np(yh, a["y"])
        e = sigmoid(yh) - (a["y"] > 0)
        assert np.isfinite(r.value) and r.value == pytest.approx(ll.mean(), rel=1e-5), (w0, r.value, ll.mean())
        assert fm.computeLogLoss(ds) == r.value
        assert st.sse == pytest.approx((e * e).sum(), rel=1e-5) and st.sum_e == pytest.approx(e.sum(), rel=1e-5, abs=1e-3)
        assert st.rows == 1500 and st.nonfinite == 0 and st.nnz == int(a["row_ptr"][-1])
    fm.w0 = a["w0"]
    f = int(a["col"][a["row_ptr"][10]])                       # a feature some rows hold
    rows_f = np.array([f in a["col"][a["row_ptr"][r]:a["row_ptr"][r + 1]] for r in range(1500)])
    assert rows_f.any() and (a["y"][rows_f] < 0).any()
    w = a["w"].copy()
    w[f] = np.inf
    fm.w = w
    r, st = C.c_double(), _ffi_stats()
    assert L().fmhip_logloss(fm.handle, ds.handle, C.byref(r), C.byref(st)) == 0
    assert st.nonfinite == int(rows_f.sum()) and np.isfinite(st.sse)
    assert not np.isfinite(r.value)
    set_loss(fm, "logistic")                                  # training stats count the same rows
    _, _, _, gst = fm.batchGradient(ds, 0)
    assert gst["nonfinite"] == int(rows_f[:500].sum())
    ds.unpersist()
    fm.close()


def _ffi_stats():
    from sparkfm_amd import _ffi
    return _ffi.Stats()


def test_refusals_and_invariance(fmhip):
    from sparkfm_amd import _ffi
    a = binary_problem(71, 600, 200, 16, 1, 20)
    # ALS: refused on a logistic model, parameters untouched
    ds1, fm = make(fmhip, a, batch_rows=0)
    set_loss(fm, "logistic")
    before = (fm.w0, fm.w.copy(), fm.v.copy())
    assert L().fmhip_als_epoch(fm.handle, ds1.handle, 0.0, 0.0, 10.0) == -5
    assert b"squared loss" in L().fmhip_last_error()
    fm._device_updated()
    assert fm.w0 == before[0] and np.array_equal(fm.w, before[1]) and np.array_equal(fm.v, before[2])
    # the scoring calls are the reference's formulas whatever the loss: the same bits
    fm2 = fmhip.FMModel(a["n1"] - 1, a["k"])
    fm2.w0, fm2.w, fm2.v = a["w0"], a["w"], a["v"]
    set_loss(fm2, "squared")

    def score(m):
        return (m.predict(ds1), m.residual(ds1), m.computeRMSE(ds1), m.termQ(ds1))
    s_sq = score(fm2)
    set_loss(fm2, "logistic")
    s_lg = score(fm2)
    for x, y in zip(s_sq, s_lg):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    ds1.unpersist()
    fm.close()
    fm2.close()
    # logistic then back to squared trains bit-identically to a model never touched; set_params / init keep the loss
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=150).cache()
    out = []
    for touch in (False, True):
        m = fmhip.FMModel(a["n1"] - 1, a["k"])
        m.w0, m.w, m.v = a["w0"], a["w"], a["v"]
        if touch:
            set_loss(m, "logistic")
            _ffi.check(L().fmhip_model_set_params(m.handle, a["w0"], _ffi.ptr(a["w"]), _ffi.ptr(np.asfortranarray(a["v"]).reshape(-1, order="F"))))
            set_loss(m, "squared")
        for _ in range(2):
            _ffi.check(L().fmhip_sgd_epoch(m.handle, ds.handle, 0.05, 0.0, 1e-3, 1e-3, None, None))
        m._device_updated()
        out.append((m.w0, m.w.copy(), m.v.copy()))
        m.close()
    assert out[0][0] == out[1][0] and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
    m = fmhip.FMModel(a["n1"] - 1, a["k"])
    m.w0, m.w, m.v = a["w0"], a["w"], a["v"]
    set_loss(m, "logistic")
    _ffi.check(L().fmhip_model_init_normal(m.handle, 5, 0.0, 0.01))
    _ffi.check(L().fmhip_model_set_params(m.handle, a["w0"], _ffi.ptr(a["w"]), _ffi.ptr(np.asfortranarray(a["v"]).reshape(-1, order="F"))))
    _, _, g0, _ = m.batchGradient(ds, 0)
    yp, e, _ = pseudo_targets(a["w0"], a["w"], a["v"], a["row_ptr"], a["col"], a["val"], a["y"], "logistic")
    assert g0 == pytest.approx(e[:150].sum(), rel=1e-5, abs=1e-4)      # still logistic
    m.close()
    ds.unpersist()


def test_logistic_fm_learns_a_classifier(fmhip):
    """A small Criteo-shaped set (2^16 rows, 2^20 slots), labels {-1,+1} split at the median: FM(...).learnWith(
    HipSGD.run(loss="logistic")) for 5 iterations.  Held-out log-loss well below the base rate's entropy, accuracy
    (the reference-faithful sign rule) above the base rate.  (The fp64 pseudo-target oracle run the same way reaches a log-loss
    of 0.85 x the entropy and an accuracy of 0.69.)"""
    from sparkfm_amd import FM, DataSet, HipSGD, synth
    n, slots = 1 << 16, 1 << 20
    d = synth.make_criteo(17, n, n_hash=slots)
    y = np.where(d["y"] > np.median(d["y"]), 1.0, -1.0).astype(np.float32)
    cut = int(n * 0.8)
    rp, col, val = d["row_ptr"], d["col"], d["val"]
    train = DataSet(rp[:cut + 1], col[:rp[cut]], val[:rp[cut]], y[:cut], batch_rows=1024)
    # held-out rows whose features the training rows span (the model is as wide as the training set's dimension)
    keep = [r for r in range(cut, n) if rp[r + 1] == rp[r] or col[rp[r]:rp[r + 1]].max() <= train.dimension]
    assert len(keep) > 0.9 * (n - cut)
    trp = np.concatenate([[0], np.cumsum(rp[np.array(keep) + 1] - rp[np.array(keep)])]).astype(np.int64)
    tcol = np.concatenate([col[rp[r]:rp[r + 1]] for r in keep])
    tval = np.concatenate([val[rp[r]:rp[r + 1]] for r in keep])
    test = DataSet(trp, tcol, tval, y[keep]).cache()
    p = float((y[keep] > 0).mean())
    base_entropy = -(p * np.log(p) + (1 - p) * np.log(1 - p))
    model = FM(train, 8, maxIteration=5, seed=3)
    fm = model.learnWith(HipSGD.run(eta=0.05, regw=1e-6, regv=1e-6, shuffle_seed=1, loss="logistic"))
    ll = fm.computeLogLoss(test)
    acc = fm.computeAccuracy(test)
    assert ll < 0.93 * base_entropy, (ll, base_entropy)
    assert acc > max(p, 1 - p) + 0.05, (acc, p)
    test.unpersist()
    fm.close()
