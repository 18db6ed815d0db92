"""Pairwise ranking (fmhip_model_set_pairing, FMHIP_PAIRING_ADJACENT; fmhip_pair_logloss): the pair residual on every training
path against the fp64 reference of train_ref.py (the unchanged oracle at the pseudo-targets y' = yhat - e), the scoring of
held-out pairs against numpy, refusals, invariance, and a ranking model that learns.

No tolerance here is new: the one-step gradient is check_grad of test_gpu_parity.py; trajectories take the bounds of
test_gpu_logistic.py (rel-L2 1e-4; data-parallel 1e-5) and test_gpu_adagrad.py (1e-5) on those tests' shapes; fmhip_pair_logloss
takes fmhip_logloss's rel 1e-5.  What IS exact under pairing is asserted exactly: sum e = 0.0."""
import ctypes as C

import numpy as np
import pytest

import oracle
import train_ref as ref
from helpers import random_problem
from test_gpu_parity import check_grad
from train_ref import DP_FRACTIONS, dp_init, dp_shard, make, rel, same

pytestmark = pytest.mark.gpu

LOG2 = float(np.log(2.0))


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def L():
    from sparkfm_amd import _ffi
    return _ffi.load()


def set_rule(fm, loss="logistic", pairs=True):
    from sparkfm_amd import _ffi
    _ffi.check(L().fmhip_model_set_loss(fm.handle, _ffi.loss_code(loss)))
    _ffi.check(L().fmhip_model_set_pairing(fm.handle, _ffi.pairing_code(pairs)))


def problem(seed, n_rows, n1, k, lo, hi, loss, empty_rows=()):
    a = random_problem(seed, n_rows, n1, k, lo, hi, empty_rows=empty_rows)
    if loss == "logistic":
        a["y"] = (np.random.default_rng(seed + 1).random(n_rows) < 0.4).astype(np.float64)      # pairs of every kind: dy in {-1, 0, 1}
    return a


def params(fm):
    return fm.w0, fm.w.copy(), fm.v.copy()


# ---- 1. fmhip_batch_grad against the reference -------------------------------------------------------------------------

def check_batches(fm, ds, a, batch_rows, loss):
    """Every batch's paired gradient against the oracle at the pseudo-targets; sum e exactly zero."""
    n = len(a["y"])
    yp, e, _ = ref.pseudo_targets(a["w0"], a["w"], a["v"], a["row_ptr"], a["col"], a["val"], a["y"], loss, True)
    assert ds.n_batches == (n + batch_rows - 1) // batch_rows > 1
    for b in range(ds.n_batches):
        r0, r1 = b * batch_rows, min(n, (b + 1) * batch_rows)
        gv, gw, g0, st = fm.batchGradient(ds, b)
        ogv, ogw, og0, osse, oe = oracle.batch_grad(a["w0"], a["w"], a["v"], r0, r1, a["row_ptr"], a["col"], a["val"], yp)
        np.testing.assert_allclose(oe, e[r0:r1], rtol=1e-12, atol=1e-12)       # the oracle's residual at y' IS the pair residual
        assert abs(og0) <= 1e-12 * np.abs(e[r0:r1]).sum()                       # (fp64: zero up to rounding)
        check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
        assert g0 == 0.0 and st["sum_e"] == 0.0                                 # fp32: zero exactly
        assert st["sse"] == pytest.approx(osse, rel=1e-5) and osse == pytest.approx(2 * (e[r0:r1:2] ** 2).sum(), rel=1e-12)
        assert st["rows"] == r1 - r0 and st["nonfinite"] == 0
        assert np.abs(ogv).max() > 0                                            # (a gradient there is)


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k", [4, 31, 32, 64, 129, 256])
def test_pair_gradient_vs_reference(fmhip, k, loss):
    """Packed rows (k < Kp: e in slot k) and full ones (k = Kp: e in the P row's low bits), every lane geometry; four batches, the
    last one short; empty rows as first, as second and as both rows of a pair (yhat = w0; d = 0 exactly for the last kind)."""
    a = problem(500 + k, 1000, 257, k, 0, 40, loss, empty_rows=(0, 17, 500, 501, 999))
    ds, fm = make(fmhip, a, batch_rows=300)
    set_rule(fm, loss)
    check_batches(fm, ds, a, 300, loss)
    ds.unpersist()
    fm.close()


def with_hot_features(a, n_rows, skip_row, seed):
    """Features 0..39 put into 10-40 % of the rows (as test_logistic_gradient_with_hot_pages builds them)."""
    rng = np.random.default_rng(seed)
    rp, cols, vals = [0], [], []
    for r in range(n_rows):
        s = slice(a["row_ptr"][r], a["row_ptr"][r + 1])
        c, x = a["col"][s], a["val"][s]
        if r != skip_row:
            hot = np.flatnonzero(rng.random(40) < np.linspace(0.4, 0.1, 40))
            keep = ~np.isin(c, hot)
            c = np.concatenate([c[keep], hot.astype(np.int32)])
            x = np.concatenate([x[keep], rng.uniform(0.2, 1.0, len(hot))])
        cols.append(c)
        vals.append(x)
        rp.append(rp[-1] + len(c))
    a.update(row_ptr=np.array(rp, np.int64), col=np.concatenate(cols).astype(np.int32), val=np.concatenate(vals))
    return a


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k", [16, 32, 64])
def test_pair_gradient_with_hot_pages(fmhip, k, loss):
    """The same with the dense hot block: the q-mode forward's prologue, the MFMA block product reading the finished P rows and e."""
    from sparkfm_amd import _ffi
    a = with_hot_features(problem(900 + k, 1200, 400, k, 3, 30, loss, empty_rows=(5,)), 1200, 5, k)
    try:
        L().fmhip_tune(_ffi.TUNE_HOT_BLOCK, 1)
        ds, fm = make(fmhip, a, batch_rows=500)
    finally:
        L().fmhip_tune(_ffi.TUNE_HOT_BLOCK, 1)
    assert len(ds.layout()["hot_ids"]) == 16                # the case is what it claims: a full two-sided page
    set_rule(fm, loss)
    check_batches(fm, ds, a, 500, loss)
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("k", [31, 64])
def test_pair_gradient_through_flat_addresses(fmhip, k):
    """The flat-address kernels (tables of 4 GiB and more; forced here by the model's tuning key), packed rows and full ones."""
    from sparkfm_amd import _ffi
    a = problem(700 + k, 800, 300, k, 0, 30, "logistic", empty_rows=(3, 400))
    ds, fm = make(fmhip, a, batch_rows=300)
    set_rule(fm, "logistic")
    _ffi.check(L().fmhip_model_tune(fm.handle, _ffi.TUNE_FLAT_ADDRESS, 1))
    check_batches(fm, ds, a, 300, "logistic")
    ds.unpersist()
    fm.close()


# ---- 2. trajectories ---------------------------------------------------------------------------------------------------

# the shapes of test_logistic_sgd_trajectory: a dense update (the merged finish: a batch touches most of the 300 rows), with
# and without decay, and a wide model (n+1 = 20000, a batch touches a few hundred rows, regv > 0: rows-only update, lazy decay)
SGD_CASES = {
    "dense_no_decay": dict(seed=31, rows=1200, n1=300, k=32, lo=2, hi=30, regs=(0.0, 0.0, 0.0), br=300, loss="logistic", tune={}),
    "dense_decay_squared": dict(seed=33, rows=1200, n1=300, k=20, lo=2, hi=30, regs=(1e-3, 1e-3, 2e-3), br=300, loss="squared", tune={}),
    "wide_lazy_decay": dict(seed=32, rows=800, n1=20000, k=64, lo=2, hi=10, regs=(1e-3, 1e-3, 2e-3), br=100, loss="logistic", tune={}),
    "wide_fused_update": dict(seed=34, rows=800, n1=20000, k=32, lo=2, hi=10, regs=(1e-3, 1e-3, 2e-3), br=100, loss="logistic",
                              tune={"FUSED_UPDATE": 1}),
}


@pytest.mark.parametrize("case", sorted(SGD_CASES))
def test_pair_sgd_trajectory(fmhip, case):
    """Two shuffled epochs of fmhip_sgd_epoch (HipSGD(pairs=True)) against the stepped reference; w0 moves by reg0 only."""
    from sparkfm_amd import _ffi
    c = SGD_CASES[case]
    a = problem(c["seed"], c["rows"], c["n1"], c["k"], c["lo"], c["hi"], c["loss"], empty_rows=(7,))
    ds, fm = make(fmhip, a, batch_rows=c["br"])
    for key, val in c["tune"].items():
        _ffi.check(L().fmhip_model_tune(fm.handle, _ffi.TUNE[key], val))
    regs = c["regs"]
    sgd = fmhip.HipSGD(eta=0.1, reg0=regs[0], regw=regs[1], regv=regs[2], shuffle_seed=11, loss=c["loss"], pairs=True)
    orders = []
    for _ in range(2):
        orders.append(sgd.batch_order(ds.n_batches).tolist())
        sgd.learn(fm, ds)
    assert sgd.last_stats["rows"] == len(a["y"]) and sgd.last_stats["sum_e"] == 0.0 and sgd.last_stats["sse"] > 0
    ow0, ow, ov = ref.epochs(ref.State(a["w0"], a["w"], a["v"]), a, c["br"], orders, 0.1, *regs, ref.Rule(c["loss"], True)).params()
    assert rel(fm.v, ov) <= 1e-4 and rel(fm.w, ow) <= 1e-4, (rel(fm.v, ov), rel(fm.w, ow))
    assert fm.w0 == pytest.approx(ow0, rel=1e-4, abs=1e-6)
    if regs[0] == 0.0:
        assert fm.w0 == np.float32(a["w0"])                    # nothing but reg0 moves the bias
    else:
        steps = 2 * ds.n_batches
        assert fm.w0 == pytest.approx(a["w0"] * (1 - 0.1 * regs[0]) ** steps, rel=1e-6)
    assert np.abs(fm.w - a["w"]).max() > 1e-3                  # it moved
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("k,loss,regs", [(32, "squared", (1e-3, 1e-3, 2e-3)), (20, "logistic", (0.0, 0.0, 0.0))])
def test_pair_adagrad_trajectory(fmhip, k, loss, regs):
    """The same under AdaGrad, on test_epochs_vs_reference's shapes and bound (1e-5, the accumulators too): with decay the dense
    pass, without it the touched rows only."""
    import test_gpu_adagrad as tga
    n1 = 500 if regs[2] else 5000
    a = problem(7 + k, 900, n1, k, 2, 20, loss)
    ds, fm = make(fmhip, a, batch_rows=200)
    sgd = fmhip.HipSGD(eta=0.05, reg0=regs[0], regw=regs[1], regv=regs[2], shuffle_seed=3, loss=loss, optimizer="adagrad", pairs=True)
    orders = []
    for _ in range(2):
        orders.append(sgd.batch_order(ds.n_batches).tolist())
        sgd.learn(fm, ds)
    assert sgd.last_stats["sum_e"] == 0.0
    s = ref.epochs(ref.State(a["w0"], a["w"], a["v"], 0.1), a, 200, orders, 0.05, *regs, ref.Rule(loss, True, tga.EPS))
    n0, nw, nv = tga.get_state(fm)
    assert rel(fm.v, s.v) <= 1e-5 and rel(fm.w, s.w) <= 1e-5, (rel(fm.v, s.v), rel(fm.w, s.w))
    assert rel(nv, s.nv) <= 1e-5 and rel(nw, s.nw) <= 1e-5, (rel(nv, s.nv), rel(nw, s.nw))
    assert fm.w0 == pytest.approx(s.w0, rel=1e-5, abs=1e-6) and n0 == pytest.approx(s.n0, rel=1e-5)
    ds.unpersist()
    fm.close()


# ---- 3. the split API --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cut", [None, 120])
def test_split_step_gives_the_bits_of_sgd_step(fmhip, cut):
    """fmhip_step_forward + fmhip_step_backward (whole, or in two feature intervals) + fmhip_step_apply == fmhip_sgd_step, bit for
    bit, on test_split_step_equals_fused_step's shape; the step's scalars carry sum e = 0."""
    from sparkfm_amd import _ffi
    a = problem(71, 900, 200, 32, 1, 20, "logistic")
    eta, regs = 0.04, (0.0, 1e-3, 1e-3)
    outs = []
    for split in (False, True):
        ds, fm = make(fmhip, a, batch_rows=300)
        set_rule(fm, "logistic")
        h, d = fm.handle, ds.handle
        for b in range(ds.n_batches):
            if not split:
                _ffi.check(L().fmhip_sgd_step(h, d, b, eta, *regs, None))
                continue
            _ffi.check(L().fmhip_step_forward(h, d, b))
            if cut is None:
                _ffi.check(L().fmhip_step_backward(h, d, b, 0, a["n1"], 1))
            else:
                _ffi.check(L().fmhip_step_backward(h, d, b, cut, a["n1"], 0))
                _ffi.check(L().fmhip_step_backward(h, d, b, 0, cut, 1))
            st = _ffi.Stats()
            _ffi.check(L().fmhip_step_stats(h, C.byref(st)))
            assert st.sum_e == 0.0 and st.sse > 0 and st.rows == 300
            _ffi.check(L().fmhip_step_apply(h, eta, *regs))
        fm._device_updated()
        outs.append(params(fm))
        ds.unpersist()
        fm.close()
    assert same(outs[0], outs[1])
    assert np.abs(outs[0][2] - a["v"]).max() > 1e-4


# ---- 4. data-parallel: thread ranks over ThreadStagedComm ----------------------------------------------------------------

DP_ROWS = [900, 600]                # even shards, even batches of 250 rows (the last ones: 150 and 100)


def dp_shards():
    return [dp_shard(4321, DP_ROWS[r], r, DP_ROWS, 800, binary=True) for r in range(2)]


@pytest.mark.parametrize("exchange", ["dense", "sharded", "touched"])
def test_pair_data_parallel(fmhip, exchange):
    """HipDataParallelSGD(loss="logistic", pairs=True), world 2, on test_logistic_data_parallel's shapes and bound: replicas
    bit-identical, the reference over the concatenated global batches matched (every rank's batch is even, so the
    concatenation keeps the pairs)."""
    from sparkfm_amd import DataSet, FMModel
    from sparkfm_amd.distributed import HipDataParallelSGD, ThreadStagedComm, run_thread_ranks
    n1, k, br, epochs = 803, 32, 250, 2
    eta, regw, regv = 0.1, 1e-3, 1e-3
    shards = dp_shards()

    def rank_fn(r, group):
        ds = DataSet.from_arrays(shards[r], batch_rows=br, device=0).cache()
        fm = FMModel(n1 - 1, k, device=0)
        fm.w0, fm.w, fm.v = dp_init(n1, k)
        comm = ThreadStagedComm(fm, r, group)
        dp = HipDataParallelSGD(comm, eta=eta, regw=regw, regv=regv, exchange=exchange, upper_fractions=DP_FRACTIONS[exchange],
                                loss="logistic", pairs=True)
        dp.plan(fm, ds)
        for _ in range(epochs):
            dp.learn(fm, ds)
        out = dict(w0=fm.w0, w=fm.w.copy(), v=fm.v.copy(), stats=dp.last_stats)
        group.barrier()
        comm.close()
        ds.unpersist()
        fm.close(discard=True)
        return out

    res = run_thread_ranks(2, rank_fn, timeout=300.0)
    assert np.array_equal(res[0]["v"], res[1]["v"]) and np.array_equal(res[0]["w"], res[1]["w"]) and res[0]["w0"] == res[1]["w0"]
    # (fmhip_dp_epoch's stats are the last global batch's summed scalars: rank 0's fourth batch alone)
    assert res[0]["stats"]["sum_e"] == 0.0 and res[0]["stats"]["sse"] > 0 and res[0]["stats"]["rows"] == 150
    w0, w, v = dp_init(n1, k)
    ow0, ow, ov = ref.dp_epochs(ref.State(w0, w, v), shards, br, [None] * epochs, eta, 0.0, regw, regv, ref.Rule("logistic", True)).params()
    assert rel(res[0]["v"], ov) <= 1e-5 and rel(res[0]["w"], ow) <= 1e-5, (rel(res[0]["v"], ov), rel(res[0]["w"], ow))
    assert res[0]["w0"] == np.float32(w0) and ow0 == pytest.approx(w0, rel=1e-12)
    assert np.abs(res[0]["w"] - w).max() > 1e-3


def test_data_parallel_plan_refusals(fmhip):
    """On EVERY rank, nobody left inside a collective: the pipelined exchange refuses a paired model at the plan
    (FMHIP_ERR_UNSUPPORTED: it runs the two-pass forward); ranks whose models differ in pairing fail the plan (the pairing travels
    in the loss's agreement word).  A pairing changed after the plan is that rank's own failure, found before the first collective."""
    from sparkfm_amd import DataSet, FMModel, _ffi
    from sparkfm_amd.distributed import HipDataParallelSGD, ThreadStagedComm, run_thread_ranks
    shards = dp_shards()

    def rank_fn(r, group):
        ds = DataSet.from_arrays(shards[r], batch_rows=250, device=0).cache()
        fm = FMModel(802, 16, device=0)
        fm.w0, fm.w, fm.v = dp_init(803, 16)
        comm = ThreadStagedComm(fm, r, group)
        out = {}

        def plan(**kw):
            try:
                HipDataParallelSGD(comm, eta=0.1, loss="logistic", **kw).plan(fm, ds)
                return 0, b""
            except _ffi.FmhipError as ex:
                return ex.code, str(ex)
        out["pipelined"] = plan(exchange="pipelined", upper_fractions=(0.1, 0.3, 0.6), pairs=True)
        out["pipelined_unpaired"] = plan(exchange="pipelined", upper_fractions=(0.1, 0.3, 0.6), pairs=False)[0]
        out["mixed"] = plan(exchange="dense", upper_fractions=(0.3,), pairs=(r == 1))
        # the same pairing everywhere: the plan passes; then rank 1 switches its pairing behind the plan's back
        out["same"] = plan(exchange="dense", upper_fractions=(0.3,), pairs=True)[0]
        if r == 1:
            _ffi.check(L().fmhip_model_set_pairing(fm.handle, _ffi.PAIRING_NONE))
        st = _ffi.Stats()
        out["epoch"] = L().fmhip_dp_epoch(fm.handle, ds.handle, comm.handle, 0.1, 0.0, 0.0, 0.0, C.byref(st))
        out["epoch_msg"] = L().fmhip_last_error()
        group.barrier()
        comm.close()
        ds.unpersist()
        fm.close(discard=True)
        return out

    res = run_thread_ranks(2, rank_fn, timeout=120.0)
    for o in res:
        assert o["pipelined"][0] == -5 and "pipelined" in o["pipelined"][1]
        assert o["pipelined_unpaired"] == 0
        assert o["mixed"][0] == -1 and "pairing" in o["mixed"][1]
        assert o["same"] == 0
        assert o["epoch"] == -1
    assert b"pairing" in res[1]["epoch_msg"]


# ---- 5. fmhip_pair_logloss -----------------------------------------------------------------------------------------------

def pair_logloss(fm, ds):
    from sparkfm_amd import _ffi
    r, c, st = C.c_double(), C.c_double(), _ffi.Stats()
    rc = L().fmhip_pair_logloss(fm.handle, ds.handle, C.byref(r), C.byref(c), C.byref(st))
    return rc, r.value, c.value, st


def concordance_slack(yh, tol):
    """Share of the pairs whose fp64 margin is within `tol` of 0 without being 0: the pairs an fp32 margin may order otherwise."""
    d = yh[0::2] - yh[1::2]
    return float(((np.abs(d) <= tol) & (d != 0)).mean())


def test_pair_logloss_vs_numpy(fmhip):
    """Mean pair log-loss (rel 1e-5, fmhip_logloss's bound) and concordance against numpy on the oracle's fp64 predictions, at the
    drawn parameters and with the linear weights scaled up (saturated margins stay finite and accurate); pairs of two empty rows
    tie (one half each).  A scoring-only dataset, several batches, any loss or pairing of the model: the same bits.  An
    infinite weight is counted in nonfinite and the mean is not finite."""
    a = problem(61, 1500, 300, 24, 0, 30, "logistic", empty_rows=(3, 10, 11, 800, 801))
    ds, fm = make(fmhip, a, batch_rows=500)
    ds_rows = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], scoring=True).cache()
    w = a["w"]
    for scale in (1.0, 60.0):
        fm.w = w * scale
        yh = oracle.predict(a["w0"], w * scale, a["v"], a["row_ptr"], a["col"], a["val"])
        ll, conc = ref.pair_scores(yh, a["y"])
        rc, r, c, st = pair_logloss(fm, ds)
        assert rc == 0 and np.isfinite(r) and r == pytest.approx(ll, rel=1e-5), (scale, r, ll)
        slack = concordance_slack(yh, 1e-5 * (1 + np.abs(yh).max()))            # TOL_Y of test_gpu_parity.py on a margin
        assert slack <= 0.005 and abs(c - conc) <= slack + 1e-15, (scale, c, conc, slack)
        e = ref.residuals(yh, a["y"], "logistic", True)
        assert st.sum_e == 0.0 and st.sse == pytest.approx((e * e).sum(), rel=1e-5)
        assert st.rows == 1500 and st.nonfinite == 0 and st.nnz == int(a["row_ptr"][-1])
        assert (fm.computePairLogLoss(ds), fm.computePairAccuracy(ds)) == (r, c)
        for loss, pairs in (("squared", True), ("logistic", False), ("logistic", True)):
            set_rule(fm, loss, pairs)
            assert pair_logloss(fm, ds)[1:3] == (r, c) and pair_logloss(fm, ds_rows)[1:3] == (r, c)
        set_rule(fm, "squared", False)
        if scale > 1:
            assert np.abs(yh[0::2] - yh[1::2]).max() > 30 and ll > 3           # the case is what it claims
    # NULL results: logloss is required, the others are not
    r = C.c_double()
    assert L().fmhip_pair_logloss(fm.handle, ds.handle, C.byref(r), None, None) == 0
    assert L().fmhip_pair_logloss(fm.handle, ds.handle, None, None, None) == -1
    fm.w = w
    f = int(a["col"][a["row_ptr"][20]])                       # a feature some rows hold
    rows_f = np.array([f in a["col"][a["row_ptr"][r]:a["row_ptr"][r + 1]] for r in range(1500)])
    assert rows_f.any()
    w2 = w.copy()
    w2[f] = np.inf
    fm.w = w2
    rc, r, c, st = pair_logloss(fm, ds)
    assert rc == 0 and st.nonfinite == int(rows_f.sum()) and not np.isfinite(r)
    set_rule(fm, "logistic", True)                            # training stats count the same rows
    _, _, _, gst = fm.batchGradient(ds, 0)
    assert gst["nonfinite"] == int(rows_f[:500].sum())
    ds.unpersist()
    ds_rows.unpersist()
    fm.close()


def test_pair_logloss_of_a_model_that_cannot_tell_the_rows_apart(fmhip):
    """All-zero parameters: every margin is 0, every pair costs log 2 — to fp64 rounding: the pairs' losses are formed and summed
    in fp64, and a sum of n equal terms in a tree of depth < 32 is off by less than 32 * 2^-53 relative (bound used: 1e-14) —
    and ties count one half: concordance 0.5 exactly.  So does any model on pairs of identical rows."""
    a = problem(62, 1000, 200, 16, 1, 20, "logistic")
    ds, fm = make(fmhip, a, batch_rows=400)
    fm.w0, fm.w, fm.v = 0.0, np.zeros_like(a["w"]), np.zeros_like(a["v"])
    rc, r, c, st = pair_logloss(fm, ds)
    assert rc == 0 and abs(r - LOG2) <= 1e-14 * LOG2 and c == 0.5
    assert st.sum_e == 0.0 and st.sse == 2 * 500 * 0.25 and st.rows == 1000 and st.nonfinite == 0
    ds.unpersist()
    twin = fmhip.DataSet.from_pairs(list(ref_rows(a, range(0, 200))), list(ref_rows(a, range(0, 200))), batch_rows=100)
    fm.w0, fm.w, fm.v = a["w0"], a["w"], a["v"]
    rc, r, c, st = pair_logloss(fm, twin)
    assert rc == 0 and abs(r - LOG2) <= 1e-14 * LOG2 and c == 0.5
    twin.unpersist()
    fm.close()


def ref_rows(a, rows):
    for r in rows:
        s = slice(a["row_ptr"][r], a["row_ptr"][r + 1])
        yield a["col"][s], a["val"][s]


# ---- 6. refusals and invariance -------------------------------------------------------------------------------------------

def test_refusals(fmhip):
    """Pairs must not straddle batches: an odd n_rows or an odd batch_rows is FMHIP_ERR_INVALID on every training call, the message
    says which, nothing changes.  ALS and the two-pass forward refuse a paired model (FMHIP_ERR_UNSUPPORTED)."""
    from sparkfm_amd import _ffi
    a = problem(71, 601, 200, 16, 1, 20, "logistic")
    even = {key: (val[:601] if key == "row_ptr" else val) for key, val in a.items()}
    even["y"] = a["y"][:600]
    even["col"], even["val"] = a["col"][:a["row_ptr"][600]], a["val"][:a["row_ptr"][600]]
    n1 = a["n1"]
    gv, gw, g0, st = np.zeros(16 * n1), np.zeros(n1), C.c_double(), _ffi.Stats()
    for data, br, word in ((a, 0, b"n_rows"), (a, 200, b"n_rows"), (even, 151, b"batch_rows")):
        ds, fm = make(fmhip, data, batch_rows=br)
        set_rule(fm, "logistic", True)
        before = params(fm)
        h, d = fm.handle, ds.handle
        calls = [lambda: L().fmhip_sgd_step(h, d, 0, 0.1, 0.0, 0.0, 0.0, None),
                 lambda: L().fmhip_sgd_epoch(h, d, 0.1, 0.0, 0.0, 0.0, None, None),
                 lambda: L().fmhip_batch_grad(h, d, 0, _ffi.ptr(gv), _ffi.ptr(gw), C.byref(g0), C.byref(st)),
                 lambda: L().fmhip_step_compute(h, d, 0),
                 lambda: L().fmhip_step_forward(h, d, 0)]
        for call in calls:
            assert call() == -1
            msg = L().fmhip_last_error()
            assert word in msg and b"odd" in msg, msg
        r = C.c_double()
        assert L().fmhip_pair_logloss(h, d, C.byref(r), None, None) == -1 and word in L().fmhip_last_error()
        fm._device_updated()
        assert same(before, params(fm))
        set_rule(fm, "logistic", False)                            # unpaired, the same dataset trains
        assert L().fmhip_sgd_step(h, d, 0, 0.1, 0.0, 0.0, 0.0, None) == 0
        ds.unpersist()
        fm.close()
    # ALS: refused on a paired (squared-loss) model, parameters untouched; the two-pass forward likewise
    ds1, fm = make(fmhip, even, batch_rows=0)
    set_rule(fm, "squared", True)
    before = params(fm)
    assert L().fmhip_als_epoch(fm.handle, ds1.handle, 0.0, 0.0, 10.0) == -5
    assert b"pairs" in L().fmhip_last_error()
    fm._device_updated()
    assert same(before, params(fm))
    _ffi.check(L().fmhip_dataset_partition_rows(ds1.handle, 100))
    for pass_ in (0, 1):
        assert L().fmhip_step_forward_pass(fm.handle, ds1.handle, 0, pass_) == -5
        assert b"two-pass" in L().fmhip_last_error()
    set_rule(fm, "squared", False)
    assert L().fmhip_als_epoch(fm.handle, ds1.handle, 0.0, 0.0, 10.0) == 0
    ds1.unpersist()
    fm.close()


def test_invariance(fmhip):
    """The scoring calls do not depend on the switch (the same bits with pairing on and off); a model switched to ADJACENT and
    back — through set_params, init_normal, set_loss and set_optimizer, none of which resets the pairing — trains bit-identically to
    one never touched; paired training is bit-identical run to run."""
    from sparkfm_amd import _ffi
    a = problem(73, 600, 200, 16, 1, 20, "logistic")
    flat_v = np.asfortranarray(a["v"]).reshape(-1, order="F")
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=150).cache()
    cands = fmhip.DataSet(a["row_ptr"][:41], a["col"][:a["row_ptr"][40]], a["val"][:a["row_ptr"][40]], a["y"][:40], scoring=True).cache()
    fm = fmhip.FMModel(a["n1"] - 1, a["k"])
    fm.w0, fm.w, fm.v = a["w0"], a["w"], a["v"]

    def score(m):
        rec = m.recommend(cands, cands, 5)
        return (m.predict(ds), m.residual(ds), m.computeRMSE(ds), m.computeLogLoss(ds), m.termQ(ds), m.computePairLogLoss(ds),
                m.computePairAccuracy(ds), m.pairScores(cands, cands), rec[0], rec[1])
    set_rule(fm, "logistic", False)
    s_off = score(fm)
    set_rule(fm, "logistic", True)
    s_on = score(fm)
    assert same(s_off, s_on)
    fm.close()
    # the switch survives the calls that set other things: the gradient is still the paired one
    m = fmhip.FMModel(a["n1"] - 1, a["k"])
    m.w0, m.w, m.v = a["w0"], a["w"], a["v"]
    set_rule(m, "squared", True)
    _ffi.check(L().fmhip_model_init_normal(m.handle, 5, 0.0, 0.01))
    _ffi.check(L().fmhip_model_set_params(m.handle, a["w0"], _ffi.ptr(a["w"]), _ffi.ptr(flat_v)))
    _ffi.check(L().fmhip_model_set_loss(m.handle, _ffi.LOSS_LOGISTIC))
    _ffi.check(L().fmhip_model_set_optimizer(m.handle, _ffi.OPT_ADAGRAD, 1e-10, 0.1))
    _ffi.check(L().fmhip_model_set_optimizer(m.handle, _ffi.OPT_SGD, 1e-10, 0.1))
    _, _, g0, st = m.batchGradient(ds, 0)
    _, e, _ = ref.pseudo_targets(a["w0"], a["w"], a["v"], a["row_ptr"], a["col"], a["val"], a["y"], "logistic", True)
    assert g0 == 0.0 and st["sse"] == pytest.approx((e[:150] ** 2).sum(), rel=1e-5)
    m.close()
    # ADJACENT and back == never touched; paired twice == paired once more
    out = {}
    for name, touch, pairs in (("plain", False, False), ("detour", True, False), ("pairs1", False, True), ("pairs2", False, True)):
        m = fmhip.FMModel(a["n1"] - 1, a["k"])
        m.w0, m.w, m.v = a["w0"], a["w"], a["v"]
        set_rule(m, "logistic", pairs)
        if touch:
            set_rule(m, "logistic", True)
            _ffi.check(L().fmhip_sgd_step(m.handle, ds.handle, 1, 0.05, 0.0, 1e-3, 1e-3, None))       # (a paired step in between)
            _ffi.check(L().fmhip_model_set_params(m.handle, a["w0"], _ffi.ptr(a["w"]), _ffi.ptr(flat_v)))
            set_rule(m, "logistic", False)
        order = np.array([2, 0, 3, 1], np.int64)
        for _ in range(2):
            _ffi.check(L().fmhip_sgd_epoch(m.handle, ds.handle, 0.05, 0.0, 1e-3, 1e-3, _ffi.ptr(order), None))
        m._device_updated()
        out[name] = params(m) + tuple(m.batchGradient(ds, 0)[:2])
        m.close()
    assert same(out["plain"], out["detour"])
    assert same(out["pairs1"], out["pairs2"])
    assert not np.array_equal(out["plain"][2], out["pairs1"][2])
    ds.unpersist()
    cands.unpersist()


# ---- 7. learning -----------------------------------------------------------------------------------------------------------

def planted_pairs(seed, users, items, n_pairs, k_true=4):
    """A planted FM over a user field (ids 0 .. users-1) and an item field (ids users .. users+items-1): score(u, i) =
    b_i + <p_u, q_i>.  A pair = one user and two items, the one the planted model scores higher first -> (preferred, other)."""
    rng = np.random.default_rng(seed)
    b = rng.normal(0, 1.0, items)
    p, q = rng.normal(0, 1.0, (users, k_true)), rng.normal(0, 0.7, (items, k_true))
    u = rng.integers(0, users, n_pairs)
    i = rng.integers(0, items, n_pairs)
    j = (i + rng.integers(1, items, n_pairs)) % items
    si, sj = b[i] + (p[u] * q[i]).sum(1), b[j] + (p[u] * q[j]).sum(1)
    first, second = np.where(si >= sj, i, j), np.where(si >= sj, j, i)
    one = np.ones(2)
    return ([(np.array([uu, users + ii], np.int32), one) for uu, ii in zip(u, first)],
            [(np.array([uu, users + jj], np.int32), one) for uu, jj in zip(u, second)])


LEARN = dict(users=200, items=120, k=8, train=4096, test=1024, batch_rows=1024, epochs=4, eta=8.0, regw=1e-4, regv=1e-4, shuffle_seed=5)


def learn_problem():
    c = LEARN
    pref, oth = planted_pairs(99, c["users"], c["items"], c["train"] + c["test"])
    n1 = c["users"] + c["items"]
    pref[0] = (np.array([pref[0][0][0], n1 - 1], np.int32), pref[0][1])     # the training rows span the model's width
    rng = np.random.default_rng(100)
    init = (0.0, np.zeros(n1), rng.normal(0, 0.1, (c["k"], n1)))
    return pref, oth, n1, init


def learn_reference(train, init, orders):
    """The fp64 reference on the same schedule -> (w0, w, v)."""
    c = LEARN
    a = dict(row_ptr=train.row_ptr, col=train.col, val=train.val, y=train.y, w0=init[0], w=init[1], v=init[2])
    return ref.epochs(ref.State(a["w0"], a["w"], a["v"]), a, c["batch_rows"], orders, c["eta"], 0.0, c["regw"], c["regv"],
                      ref.Rule("logistic", True)).params()


def test_pairwise_fm_learns_a_ranking(fmhip):
    """FM(...).learnWith(HipSGD.run(loss="logistic", pairs=True)) on pairs drawn from a planted FM.  Held-out pair log-loss ends
    below log 2 — what a model that cannot tell the rows of a pair apart scores: derived, not measured — and concordance above
    the initial model's; both within the trajectory tolerance (test_gpu_logistic.py: 1e-4) of what the fp64 reference reaches on
    the same schedule, the concordance up to the pairs whose reference margin is within that tolerance of a tie."""
    from sparkfm_amd import FM, DataSet, FMModel, HipSGD
    c = LEARN
    pref, oth, n1, init = learn_problem()
    train = DataSet.from_pairs(pref[:c["train"]], oth[:c["train"]], batch_rows=c["batch_rows"])
    test = DataSet.from_pairs(pref[c["train"]:], oth[c["train"]:]).cache()
    assert train.dimension == n1 - 1 and test.dimension <= train.dimension
    fm0 = FMModel(n1 - 1, c["k"])
    fm0.w0, fm0.w, fm0.v = init
    ll0, conc0 = fm0.computePairLogLoss(test), fm0.computePairAccuracy(test)
    fm0.close()
    sgd = HipSGD.run(eta=c["eta"], regw=c["regw"], regv=c["regv"], shuffle_seed=c["shuffle_seed"], loss="logistic", pairs=True)
    twin = HipSGD(shuffle_seed=c["shuffle_seed"])
    orders = []
    for _ in range(c["epochs"]):
        orders.append(twin.batch_order(2 * c["train"] // c["batch_rows"]).tolist())
        twin._epoch += 1
    fm = FM(train, c["k"], maxIteration=c["epochs"]).learnWith(sgd, init=init)
    ll, conc = fm.computePairLogLoss(test), fm.computePairAccuracy(test)
    assert ll < LOG2, (ll, LOG2)
    assert conc > conc0, (conc, conc0)
    ow0, ow, ov = learn_reference(train, init, orders)
    yh = oracle.predict(ow0, ow, ov, test.row_ptr, test.col, np.asarray(test.val, np.float64))
    rll, rconc = ref.pair_scores(yh, test.y)
    assert rll < LOG2 and rconc > 0.6                         # the reference itself learns on this schedule
    assert ll == pytest.approx(rll, rel=1e-4), (ll, rll)
    slack = concordance_slack(yh, 1e-4 * (1 + np.abs(yh).max()))
    assert slack <= 0.01 and abs(conc - rconc) <= slack + 1e-15, (conc, rconc, slack)
    assert abs(ll0 - LOG2) < 0.05                             # (the initial model is near the uninformed one)
    test.unpersist()
    fm.close()
