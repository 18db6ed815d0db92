"""FTRL-Proximal with L1 on every SGD training path (fmhip_model_set_ftrl, include/fmhip_ftrl.h): one step and epochs against the
fp64 twin of ftrl_ref.py (the oracle's gradient + the rule in numpy), the rows-only update against the dense one bit for bit, the
rule against AdaGrad where they coincide, the state's lifecycle, the data-parallel exchanges with thread ranks, relational data,
the sparsity counts, the public learners on a planted sparse task, and the C++ mirror.

Every comparison against fp64 starts the accumulators above zero (initial_accumulator 0.1), as test_gpu_adagrad.py's do.  The
comparison problems hold no feature seen only in single-entry rows (ftrl_ref.one_step_problem says why); the tests assert it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import ftrl_ref as fref
import relational_ref as rref
import train_ref as ref
import weight_ref as wref
from ftrl_ref import BETA, ETA, INIT, L2
from test_gpu_parity import TOL_G
from train_ref import DP_FRACTIONS, DP_ROWS, dp_init, dp_shard, make, rel, same

pytestmark = pytest.mark.gpu

STATE = ("z0", "zw", "zv", "n0", "nw", "nv")


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def L():
    from sparkfm_amd import _ffi
    return _ffi.load()


def set_ftrl(fm, beta=BETA, init=INIT, l1w=0.0, l1v=0.0):
    from sparkfm_amd import _ffi
    _ffi.check(L().fmhip_model_set_ftrl(fm.handle, beta, init, l1w, l1v))


def bits(fm):
    """Parameters and state as the device holds them (fp32 values in fp64 arrays)."""
    st = fm.ftrl_state()
    return (fm.w0, fm.w.copy(), fm.v.copy()) + tuple(st[n] for n in STATE)


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def check_step(fm, s0, s1, eta, rule):
    """The GPU's step (fm's parameters, zeta and n) against the twin's step s0 -> s1 (fp64): every change within check_step's
    per-feature tolerances of test_gpu_adagrad.py (ftrl_ref.tolerances), the device starting from the fp32 values of s0 and from the
    fp32 expression of zeta.  The zero pattern matches exactly except at coordinates whose twin |zeta'| lies within zeta's tolerance
    of tau, and those are at most 1 % of the touched ones (theta is not compared there: 0 on one side, a sliver on the other)."""
    st = fm.ftrl_state()
    tol = fref.tolerances(s0, s1)
    near = fref.near_threshold(s0, s1, eta, rule)
    z_start = {"zv": fref.zeta_init(s0.v, s0.nv, rule.beta, np.float32), "zw": fref.zeta_init(s0.w, s0.nw, rule.beta, np.float32)}
    got = {"v": fm.v, "w": fm.w, "zv": st["zv"], "zw": st["zw"], "nv": st["nv"], "nw": st["nw"]}
    for name in ("v", "w", "zv", "zw", "nv", "nw"):
        start = z_start[name].astype(np.float64) if name in z_start else f32(getattr(s0, name))
        d_ref = getattr(s1, name) - getattr(s0, name)
        err = np.abs((got[name] - start) - d_ref)
        keep = ~near[name[-1]] if name in ("v", "w") else np.ones(err.shape, bool)
        print("%s: largest error / tolerance %.3g" % (name, float((err / tol[name])[keep].max())))
        assert (err <= tol[name])[keep].all(), (name, float((err / tol[name])[keep].max()))
    for name, g in (("w", s1.g[1]), ("v", s1.g[2])):
        touched = g != 0
        zero_dev, zero_ref = (got[name] == 0) & touched, (getattr(s1, name) == 0) & touched
        share = zero_ref.sum() / max(touched.sum(), 1)
        print("%s: %d touched, %.3f of them zero in the twin, %d near the threshold, %d differ" % (
            name, touched.sum(), share, near[name].sum(), (zero_dev != zero_ref).sum()))
        if getattr(rule, "l1" + name) > 0:
            assert 0.3 <= share <= 0.7, (name, share)
        assert not ((zero_dev != zero_ref) & ~near[name]).any(), name
        assert near[name].sum() <= fref.ZERO_CAP * touched.sum(), (name, int(near[name].sum()), int(touched.sum()))
        assert not np.signbit(got[name][zero_dev]).any()                    # exactly +0
    assert fm.w0 - f32(s0.w0) == pytest.approx(s1.w0 - s0.w0, rel=2 * TOL_G, abs=1.2e-7 * abs(s1.w0) + 1e-9)
    assert st["n0"] - f32(s0.n0) == pytest.approx(s1.n0 - s0.n0, rel=2 * TOL_G, abs=3e-7 * s1.n0)
    assert st["z0"] - float(fref.zeta_init(s0.w0, s0.n0, rule.beta, np.float32)) == pytest.approx(s1.z0 - s0.z0, rel=2 * TOL_G,
                                                                                                  abs=1.2e-7 * abs(s1.z0) + 1e-9)


# ---- 1. one step against the twin -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k", fref.KS)
@pytest.mark.parametrize("path", ["dense", "rows"])
def test_one_step_vs_twin(fmhip, k, loss, path):
    """fmhip_sgd_step under FTRL with L1 and L2 on: V, w, w0 with their zeta and n.  dense: the whole model is walked (k_apply);
    rows: a model far wider than the batch (k_apply_rows on the touched rows only, WITH l1 and l2 > 0 — the others must not move a
    bit).  l1w / l1v come from the twin: the median |zeta'| of the touched coordinates."""
    a = fref.one_step_problem(k, loss, path)
    assert len(fref.cancelling_features(a["row_ptr"], a["col"], a["n1"])) == 0
    l1w, l1v = fref.choose_l1(a, loss)
    rule = fref.Rule(loss, False, BETA, l1w, l1v)
    ds, fm = make(fmhip, a, batch_rows=0, loss=loss)
    s0 = fref.State(a["w0"], a["w"], a["v"], INIT, BETA)
    s1 = fref.step(s0.copy(), a["row_ptr"], a["col"], a["val"], a["y"], 0, len(a["y"]), ETA, *L2, rule)
    learner = fmhip.HipFTRL(alpha=ETA, beta=BETA, l1w=l1w, l1v=l1v, l2_0=L2[0], l2w=L2[1], l2v=L2[2], ftrl_init=INIT, loss=loss)
    learner.step(fm, ds, 0)
    check_step(fm, s0, s1, ETA, rule)
    if path == "rows":
        untouched = np.setdiff1d(np.arange(a["n1"]), a["col"])
        assert len(untouched) > a["n1"] // 2
        st = fm.ftrl_state()
        f0 = fref.State(a["w0"], a["w"], a["v"], INIT, BETA, np.float32)
        for got, want in ((fm.v, f0.v), (st["zv"], f0.zv), (st["nv"], f0.nv)):
            assert np.array_equal(got[:, untouched], want[:, untouched].astype(np.float64))
        for got, want in ((fm.w, f0.w), (st["zw"], f0.zw), (st["nw"], f0.nw)):
            assert np.array_equal(got[untouched], want[untouched].astype(np.float64))
    ds.unpersist()
    fm.close()


# ---- 2. rows-only == dense, bit for bit ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [8, 32, 100])
def test_rows_only_equals_dense_bitwise(fmhip, k):
    """The same wide batch through fmhip_sgd_step (its update: k_apply_rows over the touched rows) and through fmhip_step_compute +
    fmhip_step_apply (k_apply over the whole model), L1 and L2 on: theta, zeta and n are equal bit for bit — a row without a gradient
    does not move under this rule, whatever the regularisation."""
    from sparkfm_amd import _ffi
    a = fref.one_step_problem(k, "logistic", "rows")
    l1w, l1v = fref.choose_l1(a, "logistic")
    outs = []
    for dense in (False, True):
        ds, fm = make(fmhip, a, batch_rows=0, loss="logistic")
        set_ftrl(fm, BETA, INIT, l1w, l1v)
        if dense:
            _ffi.check(L().fmhip_step_compute(fm.handle, ds.handle, 0))
            _ffi.check(L().fmhip_step_apply(fm.handle, ETA, *L2))
        else:
            _ffi.check(L().fmhip_sgd_step(fm.handle, ds.handle, 0, ETA, *L2, None))
        fm._device_updated()
        outs.append(bits(fm))
        ds.unpersist()
        fm.close()
    assert same(outs[0], outs[1])
    assert (outs[0][2] == 0).any() and not np.array_equal(outs[0][2], f32(a["v"]))


# ---- 3. epochs against the twin -----------------------------------------------------------------------------------------------

def check_epochs(fm, s):
    """test_gpu_adagrad.test_epochs_vs_reference's tolerances: relative L2 error 1e-5, on the parameters and on the state."""
    st = fm.ftrl_state()
    errs = dict(v=rel(fm.v, s.v), w=rel(fm.w, s.w), zv=rel(st["zv"], s.zv), zw=rel(st["zw"], s.zw), nv=rel(st["nv"], s.nv), nw=rel(st["nw"], s.nw))
    print(errs)
    assert max(errs.values()) <= 1e-5, errs
    assert fm.w0 == pytest.approx(s.w0, rel=1e-5, abs=1e-6) and st["n0"] == pytest.approx(s.n0, rel=1e-5)
    assert st["z0"] == pytest.approx(s.z0, rel=1e-5, abs=1e-6)


@pytest.mark.parametrize("case", ["single", "pairs", "weighted"])
def test_epochs_vs_twin(fmhip, case):
    """800 rows x 300 features, 4 batches, 3 shuffled epochs, k = 20, logistic, L1 and L2 on (HipFTRL.learn); pairs: the rows as
    DataSet.from_pairs interleaves them; weighted: example weights from weight_ref — the same twin over train_ref's pair and
    weight_ref's weighted residuals."""
    k = 20
    a = fref.problem(7 + k, 800, 300, k, 2, 20, "logistic")
    assert len(fref.cancelling_features(a["row_ptr"], a["col"], a["n1"])) == 0
    c = wref.draw_weights(5, 800) if case == "weighted" else None
    if case == "pairs":
        rows = list(zip(np.split(a["col"], a["row_ptr"][1:-1]), np.split(a["val"], a["row_ptr"][1:-1])))
        ds = fmhip.DataSet.from_pairs(rows[0::2], rows[1::2], batch_rows=200).cache()
        a = dict(a, y=np.tile([1.0, 0.0], 400))
    else:
        ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=200, weights=c).cache()
    fm = fmhip.FMModel(a["n1"] - 1, k)
    fm.w0, fm.w, fm.v = a["w0"], a["w"], a["v"]
    l1w, l1v = 0.1, 0.01
    learner = fmhip.HipFTRL.run(alpha=ETA, beta=BETA, l1w=l1w, l1v=l1v, l2_0=L2[0], l2w=L2[1], l2v=L2[2], ftrl_init=INIT, loss="logistic",
                                pairs=case == "pairs", shuffle_seed=3)
    orders = []
    for _ in range(3):
        orders.append(learner.batch_order(ds.n_batches).tolist())
        learner.learn(fm, ds)
    s = fref.epochs(fref.State(a["w0"], a["w"], a["v"], INIT, BETA), a, 200, orders, ETA, *L2,
                    fref.Rule("logistic", case == "pairs", BETA, l1w, l1v), c)
    check_epochs(fm, s)
    assert (s.w == 0).any() and (s.v == 0).any() and (s.w != 0).any() and (s.v != 0).any()
    ds.unpersist()
    fm.close()


# ---- 4. AdaGrad where the two rules coincide ---------------------------------------------------------------------------------

def test_without_l1_l2_is_adagrad_on_the_device(fmhip):
    """l1 = l2 = 0, beta = 1e-3, accumulators from 0.1, 5 steps: the FTRL model and an AdaGrad model (eps = 1e-3) are each within
    1e-5 (rel L2) of their twins, which are equal (1e-12), and so within 2e-5 of each other."""
    k, eps = 20, 1e-3
    a = fref.problem(31, 1000, 300, k, 2, 20, "logistic")
    out = {}
    for which in ("ftrl", "adagrad"):
        ds, fm = make(fmhip, a, batch_rows=200, loss="logistic")
        if which == "ftrl":
            fmhip.HipFTRL(alpha=ETA, beta=eps, ftrl_init=INIT, loss="logistic").learn(fm, ds)
        else:
            fmhip.HipSGD(eta=ETA, loss="logistic", optimizer="adagrad", adagrad_eps=eps, adagrad_init=INIT).learn(fm, ds)
        out[which] = (fm.w0, fm.w.copy(), fm.v.copy())
        ds.unpersist()
        fm.close()
    sf = fref.epochs(fref.State(a["w0"], a["w"], a["v"], INIT, eps), a, 200, [None], ETA, 0.0, 0.0, 0.0, fref.Rule("logistic", False, eps))
    sa = ref.epochs(ref.State(a["w0"], a["w"], a["v"], INIT), a, 200, [None], ETA, 0.0, 0.0, 0.0, ref.Rule("logistic", False, eps))
    assert rel(sf.v, sa.v) <= 1e-12 and rel(sf.w, sa.w) <= 1e-12 and abs(sf.w0 - sa.w0) <= 1e-12
    for which, s in (("ftrl", sf), ("adagrad", sa)):
        errs = (rel(out[which][2], s.v), rel(out[which][1], s.w))
        print(which, errs)
        assert max(errs) <= 1e-5 and out[which][0] == pytest.approx(s.w0, rel=1e-5, abs=1e-6), (which, errs)
    assert rel(out["ftrl"][2], out["adagrad"][2]) <= 2e-5 and rel(out["ftrl"][1], out["adagrad"][1]) <= 2e-5


# ---- 5. the state's lifecycle --------------------------------------------------------------------------------------------------

def test_state_lifecycle(fmhip):
    from sparkfm_amd import _ffi
    a = fref.problem(17, 500, 400, 24, 2, 20, "squared")
    ds, fm = make(fmhip, a, batch_rows=200)
    z0 = C.c_double()
    assert L().fmhip_model_get_ftrl_state(fm.handle, C.byref(z0), None, None, None, None, None) == -1       # SGD: no state
    set_ftrl(fm, 0.5, 0.25, 0.01, 0.001)
    f0 = fref.State(a["w0"], a["w"], a["v"], 0.25, 0.5, np.float32)
    st = fm.ftrl_state()
    assert st["n0"] == 0.25 and (st["nw"] == 0.25).all() and (st["nv"] == 0.25).all()
    assert np.array_equal(st["zv"], f0.zv.astype(np.float64)) and np.array_equal(st["zw"], f0.zw.astype(np.float64)) and st["z0"] == float(f0.z0)
    learner = fmhip.HipFTRL(alpha=ETA, beta=0.5, l1w=0.01, l1v=0.001, l2w=1e-3, l2v=1e-3, ftrl_init=0.25)
    learner.learn(fm, ds)
    s1 = bits(fm)
    assert (s1[8] > 0.25).any()
    set_ftrl(fm, 0.5, 0.25, 0.01, 0.001)                          # the same settings again: a no-op that keeps the state
    assert same(s1, bits(fm))
    # the model's own values written back keep the state (bit-equal parameters still agree with their zeta) ...
    _ffi.check(L().fmhip_model_set_params(fm.handle, s1[0], _ffi.ptr(np.ascontiguousarray(s1[1])), _ffi.ptr(np.ascontiguousarray(s1[2].reshape(-1, order="F")))))
    assert same(s1, bits(fm))
    # ... and new parameters re-derive zeta from them and the current n: the fp32 expression
    fm.w0, fm.w, fm.v = 0.3, a["w"] * 2 + 0.01, a["v"] * 3 + 0.01
    st = fm.ftrl_state()
    assert np.array_equal(st["nv"], s1[8]) and np.array_equal(st["nw"], s1[7])
    assert np.array_equal(st["zv"], fref.zeta_init(f32(fm.v), st["nv"], 0.5, np.float32).astype(np.float64))
    assert np.array_equal(st["zw"], fref.zeta_init(f32(fm.w), st["nw"], 0.5, np.float32).astype(np.float64))
    assert st["z0"] == float(fref.zeta_init(np.float32(0.3), st["n0"], 0.5, np.float32))
    _ffi.check(L().fmhip_model_init_normal(fm.handle, 5, 0.0, 0.05))
    fm._device_updated()
    st = fm.ftrl_state()
    assert np.array_equal(st["zv"], fref.zeta_init(f32(fm.v), st["nv"], 0.5, np.float32).astype(np.float64)) and (fm.v != 0).all()
    assert (st["zw"] == 0).all() and st["z0"] == 0 and np.array_equal(st["nv"], s1[8])
    set_ftrl(fm, 0.5, 0.5, 0.01, 0.001)                           # other settings: a fresh state
    assert (fm.ftrl_state()["nv"] == 0.5).all()
    set_ftrl(fm, 0.5, 0.5, 0.02, 0.001)
    assert (fm.ftrl_state()["nv"] == 0.5).all()
    # get / set round trip, and what the setter refuses
    fmhip.HipFTRL(alpha=ETA, beta=0.5, l1w=0.02, l1v=0.001, ftrl_init=0.5).learn(fm, ds)
    st = fm.ftrl_state()
    fm.set_ftrl_state(dict(z0=-1.5, zw=np.full_like(st["zw"], -2.0), zv=np.full_like(st["zv"], 3.0), n0=1.5, nw=np.full_like(st["nw"], 2.0),
                           nv=np.full_like(st["nv"], 4.0)))
    t = fm.ftrl_state()
    assert (t["z0"], t["n0"]) == (-1.5, 1.5) and (t["zw"] == -2.0).all() and (t["zv"] == 3.0).all() and (t["nw"] == 2.0).all() and (t["nv"] == 4.0).all()
    fm.set_ftrl_state(st)
    assert same([st[n] for n in STATE], [fm.ftrl_state()[n] for n in STATE])
    for name, bad in (("nv", -1.0), ("nv", np.nan), ("nw", np.inf), ("zv", np.nan), ("zw", np.inf)):
        broken = dict(st, **{name: st[name].copy()})
        broken[name].flat[0] = bad
        with pytest.raises(_ffi.FmhipError) as ei:
            fm.set_ftrl_state(broken)
        assert ei.value.code == -1 and name in str(ei.value)
    assert same([st[n] for n in STATE], [fm.ftrl_state()[n] for n in STATE])
    # the AdaGrad state calls refuse an FTRL model; SGD frees the state, and the FTRL state calls are then INVALID
    n0 = C.c_double()
    assert L().fmhip_model_get_optimizer_state(fm.handle, C.byref(n0), None, None) == -1
    _ffi.check(L().fmhip_model_set_optimizer(fm.handle, _ffi.OPT_SGD, 0.0, 0.0))
    assert L().fmhip_model_get_ftrl_state(fm.handle, C.byref(z0), None, None, None, None, None) == -1
    with pytest.raises(_ffi.FmhipError):
        fm.set_ftrl_state(st)
    # AdaGrad after FTRL starts from AdaGrad's own accumulators
    set_ftrl(fm, 0.5, 0.5)
    _ffi.check(L().fmhip_model_set_optimizer(fm.handle, _ffi.OPT_ADAGRAD, 1e-10, 0.125))
    nv = np.zeros(fm.num_factor * (fm.num_attribute + 1))
    _ffi.check(L().fmhip_model_get_optimizer_state(fm.handle, C.byref(n0), None, _ffi.ptr(nv)))
    assert n0.value == 0.125 and (nv == 0.125).all()
    assert L().fmhip_model_get_ftrl_state(fm.handle, C.byref(z0), None, None, None, None, None) == -1
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("regs", [(1e-3, 1e-3, 2e-3), (0.0, 0.0, 0.0)])
def test_sgd_after_ftrl_trains_as_a_model_that_never_was(fmhip, regs):
    from sparkfm_amd import _ffi
    a = fref.problem(23, 500, 3000, 16, 2, 20, "squared")
    outs = []
    for detour in (False, True):
        ds, fm = make(fmhip, a, batch_rows=200)
        if detour:
            set_ftrl(fm, 0.5, 0.1, 0.01, 0.01)
            _ffi.check(L().fmhip_model_set_optimizer(fm.handle, _ffi.OPT_SGD, 0.0, 0.0))
        fmhip.HipSGD(eta=0.05, reg0=regs[0], regw=regs[1], regv=regs[2]).learn(fm, ds)
        outs.append((fm.w0, fm.w.copy(), fm.v.copy()))
        ds.unpersist()
        fm.close()
    assert same(outs[0], outs[1])


@pytest.mark.parametrize("k", [32, 40])
def test_resume_is_bitwise(fmhip, k):
    """Two epochs in a row == one epoch, then parameters + state copied into a FRESH model (set_params, set_ftrl, set_ftrl_state),
    then the second epoch — bit for bit (accumulators started at 0: GPU against GPU)."""
    a = fref.problem(29, 600, 2500, k, 2, 20, "squared")
    kw = dict(alpha=0.05, beta=0.5, l1w=0.01, l1v=0.001, l2w=1e-3, l2v=2e-3, ftrl_init=0.0)
    ds, fm = make(fmhip, a, batch_rows=200)
    fmhip.HipFTRL(**kw).learn(fm, ds)
    mid = bits(fm)
    fmhip.HipFTRL(**kw).learn(fm, ds)
    straight = bits(fm)
    fm.close()
    fm2 = fmhip.FMModel(a["n1"] - 1, k)
    fm2.w0, fm2.w, fm2.v = mid[0], mid[1], mid[2]
    set_ftrl(fm2, 0.5, 0.0, 0.01, 0.001)
    fm2.set_ftrl_state(dict(zip(STATE, mid[3:])))
    fmhip.HipFTRL(**kw).learn(fm2, ds)
    assert same(straight, bits(fm2))
    assert not same(mid[:3], straight[:3])
    ds.unpersist()
    fm2.close()


# ---- 6. data-parallel, thread ranks on one GPU ------------------------------------------------------------------------------

DP_L1 = (0.1, 0.01)


def dp_run(world, exchange, shards, n1, k, br, epochs, orders=None, l1w_of=None):
    from sparkfm_amd import DataSet, FMModel, HipDataParallelFTRL
    from sparkfm_amd.distributed import ThreadStagedComm, run_thread_ranks

    def rank_fn(r, group):
        ds = DataSet.from_arrays(shards[r], batch_rows=br, device=0).cache()
        fm = FMModel(n1 - 1, k, device=0)
        fm.w0, fm.w, fm.v = dp_init(n1, k)
        comm = ThreadStagedComm(fm, r, group)
        dp = HipDataParallelFTRL(comm, alpha=ETA, beta=BETA, l1w=DP_L1[0] if l1w_of is None else l1w_of(r), l1v=DP_L1[1], l2_0=L2[0], l2w=L2[1],
                                 l2v=L2[2], ftrl_init=INIT, exchange=exchange, upper_fractions=DP_FRACTIONS[exchange])
        out = {}
        try:
            dp.plan(fm, ds)
            for e in range(epochs):
                dp.learn(fm, ds, order=None if orders is None else orders[e])
            out = dict(bits=bits(fm), rc=0)
        except Exception as ex:           # noqa: BLE001 — the refusals are what some cases test
            out = dict(rc=getattr(ex, "code", "?"), msg=str(ex))
        group.barrier()
        comm.close()
        ds.unpersist()
        fm.close(discard=True)
        return out

    return run_thread_ranks(world, rank_fn, timeout=300.0)


@pytest.mark.parametrize("world,exchange,shuffle", [(2, "dense", False), (8, "dense", False), (2, "pipelined", True), (8, "pipelined", True),
                                                    (2, "touched", False), (8, "touched", False)])
def test_ftrl_data_parallel(fmhip, world, exchange, shuffle):
    """HipDataParallelFTRL with l1 > 0 and l2 > 0 on every exchange that takes the rule — the touched one included, on a model five
    times wider than the data: every replica (parameters, zeta and n) bitwise equal to rank 0's, and the twin over the global
    batches matched within rel-L2 1e-5."""
    rows, n1_data, k, br, epochs = DP_ROWS[world], 800, 32, 250, 2
    n1 = 803 if exchange != "touched" else 4003
    shards = [dp_shard(4321, rows[r], r, rows, n1_data) for r in range(world)]
    steps = max((len(d["y"]) + br - 1) // br for d in shards)
    orders = [np.random.default_rng(e).permutation(steps).tolist() for e in range(epochs)] if shuffle else None
    res = dp_run(world, exchange, shards, n1, k, br, epochs, orders)
    assert all(o["rc"] == 0 for o in res), [o.get("msg") for o in res]
    for r in range(1, world):
        assert same(res[0]["bits"], res[r]["bits"]), r
    w0, w, v = dp_init(n1, k)
    s = fref.dp_epochs(fref.State(w0, w, v, INIT, BETA), shards, br, orders or [None] * epochs, ETA, *L2,
                       fref.Rule("squared", False, BETA, *DP_L1))
    got = dict(zip(("w0", "w", "v") + STATE, res[0]["bits"]))
    errs = {n: rel(got[n], getattr(s, n)) for n in ("w", "v", "zw", "zv", "nw", "nv")}
    print(errs)
    assert max(errs.values()) <= 1e-5, errs
    assert abs(got["w0"] - s.w0) <= 1e-5 * abs(s.w0) + 1e-6
    if exchange == "touched":       # the rows no rank ever touched hold their first bits
        f0 = fref.State(w0, w, v, INIT, BETA, np.float32)
        assert np.array_equal(got["v"][:, n1_data:], f0.v[:, n1_data:].astype(np.float64))
        assert np.array_equal(got["zv"][:, n1_data:], f0.zv[:, n1_data:].astype(np.float64)) and (got["nv"][:, n1_data:] == np.float32(INIT)).all()


@pytest.mark.parametrize("world", [2, 8])
def test_ftrl_sharded_exchange_is_refused_on_every_rank(fmhip, world):
    rows = DP_ROWS[world]
    shards = [dp_shard(99, rows[r], r, rows, 300) for r in range(world)]
    res = dp_run(world, "sharded", shards, 303, 16, 250, 1)
    assert [o["rc"] for o in res] == [-5] * world, [o.get("msg") for o in res]
    assert all("FTRL" in o["msg"] for o in res), res[0]["msg"]


@pytest.mark.parametrize("world", [2, 8])
def test_ranks_that_disagree_on_l1w_are_refused_by_the_plan(fmhip, world):
    rows = DP_ROWS[world]
    shards = [dp_shard(98, rows[r], r, rows, 300) for r in range(world)]
    res = dp_run(world, "dense", shards, 303, 16, 250, 1, l1w_of=lambda r: 0.03 if r == world - 1 else 0.02)
    assert [o["rc"] for o in res] == [-1] * world, [o.get("msg") for o in res]
    assert all("fmhip_model_set_ftrl" in o["msg"] and "l1w" in o["msg"] for o in res), res[0]["msg"]


@pytest.mark.parametrize("field", ["l1v", "beta", "to_adagrad"])
def test_rule_changed_after_the_plan_is_that_ranks_failure(fmhip, field):
    """Two ranks plan under FTRL, then rank 1 alone changes its rule and both take fmhip_dp_step_at(0): rank 1 is refused
    (FMHIP_ERR_INVALID naming the planned and the present settings, the setter, and the way out) but has taken the step's collectives
    with a zero contribution — rank 0's step completes, and both ranks issued the same (kind, count) sequence."""
    from sparkfm_amd import DataSet, FMModel, _ffi
    from sparkfm_amd.distributed import ThreadStagedComm, run_thread_ranks
    rows = [64, 64]
    shards = [dp_shard(97, rows[r], r, rows, 100) for r in range(2)]

    def rank_fn(r, group):
        ds = DataSet.from_arrays(shards[r], batch_rows=32, device=0).cache()
        fm = FMModel(100, 8, device=0)
        fm.w0, fm.w, fm.v = dp_init(101, 8)
        comm = ThreadStagedComm(fm, r, group)
        lib = L()
        set_ftrl(fm, 0.5, 0.1, 0.02, 0.002)
        fr = np.array([0.3])
        _ffi.check(lib.fmhip_dp_plan(fm.handle, ds.handle, comm.handle, 1, _ffi.ptr(fr), None))
        if r == 1:
            if field == "to_adagrad":
                _ffi.check(lib.fmhip_model_set_optimizer(fm.handle, _ffi.OPT_ADAGRAD, 1e-10, 0.1))
            else:
                set_ftrl(fm, 0.25 if field == "beta" else 0.5, 0.1, 0.02, 0.004 if field == "l1v" else 0.002)
        before = len(comm.calls)
        rc = lib.fmhip_dp_step_at(fm.handle, ds.handle, 0, comm.handle, 0.05, 0.0, 1e-3, 1e-3)
        out = dict(rc=rc, msg=lib.fmhip_last_error().decode() if rc else "", calls=comm.calls[before:])
        group.barrier()
        comm.close()
        ds.unpersist()
        fm.close(discard=True)
        return out

    res = run_thread_ranks(2, rank_fn, timeout=60.0)
    assert res[0]["rc"] == 0, res[0]["msg"]
    assert res[1]["rc"] == -1
    names = {"l1v": ["l1v 0.002", "l1v 0.004"], "beta": ["beta 0.5", "beta 0.25"], "to_adagrad": ["optimizer 2", "optimizer 1"]}[field]
    for name in names + ["fmhip_model_set_ftrl", "call fmhip_dp_plan again (every rank)", "contributed zeros"]:
        assert name in res[1]["msg"], (name, res[1]["msg"])
    assert res[0]["calls"] == res[1]["calls"] and len(res[0]["calls"]) >= 2


# ---- 7. relational data -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k", [8, 32, 100])
def test_relational_step_vs_the_flat_step(fmhip, k, loss):
    """HipFTRL.step on a RelationalData against the twin's step on the expanded rows (check_step: test_gpu_relational.py's one-step
    tolerance is the same per-feature TOL_G), and against the device's own flat step on expand(): within twice that tolerance of
    each other (two fp32 paths), zero pattern as in test 1."""
    p = rref.base_problem(500 + k, k, loss)
    a = rref.flat(p)
    assert len(fref.cancelling_features(a["row_ptr"], a["col"], a["n1"])) == 0
    l1w, l1v = fref.choose_l1(a, loss)
    rule = fref.Rule(loss, False, BETA, l1w, l1v)
    s0 = fref.State(a["w0"], a["w"], a["v"], INIT, BETA)
    s1 = fref.step(s0.copy(), a["row_ptr"], a["col"], a["val"], a["y"], 0, len(a["y"]), ETA, *L2, rule)
    kw = dict(alpha=ETA, beta=BETA, l1w=l1w, l1v=l1v, l2_0=L2[0], l2w=L2[1], l2v=L2[2], ftrl_init=INIT, loss=loss)
    rd, fm = rref.build(fmhip, p)
    fmhip.HipFTRL(**kw).step(fm, rd, 0)
    check_step(fm, s0, s1, ETA, rule)
    fl = rd.expand().cache()
    fm2 = fmhip.FMModel(p["n1"] - 1, k)
    fm2.w0, fm2.w, fm2.v = p["w0"], p["w"], p["v"]
    fmhip.HipFTRL(**kw).step(fm2, fl, 0)
    check_step(fm2, s0, s1, ETA, rule)
    tol = fref.tolerances(s0, s1)
    near = fref.near_threshold(s0, s1, ETA, rule)
    assert (np.abs(fm.v - fm2.v) <= 2 * tol["v"])[~near["v"]].all() and (np.abs(fm.w - fm2.w) <= 2 * tol["w"])[~near["w"]].all()
    fl.unpersist()
    fm2.close()
    rd.unpersist()
    for part in rd._parts():
        part.unpersist()
    fm.close()


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k", [8, 32, 100])
def test_relational_step_with_hot_block_parts_vs_the_flat_step(fmhip, k, loss):
    """test_relational_step_vs_the_flat_step on relational_ref.base_problem(hot=True): the user block built with a dense hot block
    by name, the plain part in four batches with one of its own (asserted) — every batch's step against the twin and against the
    flat step on expand(), the same tolerances and caps; two runs bit-identical."""
    p = rref.base_problem(700 + k, k, loss, hot=True)
    a, br = rref.flat(p), 100
    assert len(fref.cancelling_features(a["row_ptr"], a["col"], a["n1"])) == 0
    l1w, l1v = fref.choose_l1(a, loss)
    rule = fref.Rule(loss, False, BETA, l1w, l1v)
    s0 = fref.State(a["w0"], a["w"], a["v"], INIT, BETA)
    kw = dict(alpha=ETA, beta=BETA, l1w=l1w, l1v=l1v, l2_0=L2[0], l2w=L2[1], l2v=L2[2], ftrl_init=INIT, loss=loss)
    want_u, want_p = rref.hot_layouts(p, br)
    for b in range(4):
        s1 = fref.step(s0.copy(), a["row_ptr"], a["col"], a["val"], a["y"], b * br, (b + 1) * br, ETA, *L2, rule)
        outs = []
        for _ in range(2):
            rd, fm = rref.build(fmhip, p, br, hot_block=4)
            fmhip.HipFTRL(**kw).step(fm, rd, b)
            outs.append(bits(fm))
            got_u, got_p = rd.relations[0].block.layout(), rd.plain.layout()
            assert got_u["hot_pages"] == want_u["hot_pages"] >= 1 and sorted(got_u["hot_ids_all"]) == want_u["hot_ids_all"]
            assert got_p["hot_pages"] == want_p["hot_pages"] >= 1 and sorted(got_p["hot_ids_all"]) == want_p["hot_ids_all"]
            if len(outs) == 1:
                check_step(fm, s0, s1, ETA, rule)
                fl = rd.expand().cache()
                fm2 = fmhip.FMModel(p["n1"] - 1, k)
                fm2.w0, fm2.w, fm2.v = p["w0"], p["w"], p["v"]
                fmhip.HipFTRL(**kw).step(fm2, fl, b)
                check_step(fm2, s0, s1, ETA, rule)
                tol = fref.tolerances(s0, s1)
                near = fref.near_threshold(s0, s1, ETA, rule)
                assert (np.abs(fm.v - fm2.v) <= 2 * tol["v"])[~near["v"]].all() and (np.abs(fm.w - fm2.w) <= 2 * tol["w"])[~near["w"]].all()
                fl.unpersist()
                fm2.close()
            rd.unpersist()
            for part in rd._parts():
                part.unpersist()
            fm.close()
        assert same(outs[0], outs[1]), b


# ---- 8. the sparsity counts ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [8, 32])
def test_nonzeros_equal_numpy_counts(fmhip, k):
    """fmhip_model_nonzeros against numpy over get_params: k = 8 (padded rows, w in the packed slot) and k = 32 (w beside the table);
    2701 features: several blocks, a row count that is no multiple of anything; -0 counts as zero."""
    rng = np.random.default_rng(k)
    n1 = 2701
    fm = fmhip.FMModel(n1 - 1, k)
    w = rng.normal(0, 1, n1) * (rng.random(n1) < 0.3)
    v = rng.normal(0, 1, (k, n1)) * (rng.random((k, n1)) < 0.2)
    dead = rng.random(n1) < 0.25
    v[:, dead] = 0.0
    w[dead[::-1]] = 0.0
    w[5], v[0, 7] = -0.0, -0.0
    fm.w0, fm.w, fm.v = 0.5, w, v
    got = fm.nonzeros()
    gw, gv = f32(fm.w), f32(fm.v)
    want = dict(w_nonzero=int((gw != 0).sum()), v_nonzero=int((gv != 0).sum()), features_all_zero=int(((gw == 0) & (gv == 0).all(axis=0)).sum()),
                w_total=n1, v_total=n1 * k)
    assert got == want and 0 < want["features_all_zero"] < n1 and want["w_nonzero"] > 0
    fm.w, fm.v = np.zeros(n1), np.zeros((k, n1))
    assert fm.nonzeros() == dict(w_nonzero=0, v_nonzero=0, features_all_zero=n1, w_total=n1, v_total=n1 * k)
    fm.v = np.ones((k, n1))
    assert fm.nonzeros() == dict(w_nonzero=0, v_nonzero=n1 * k, features_all_zero=0, w_total=n1, v_total=n1 * k)
    fm.close()


# ---- 9. through the public flow: a planted sparse task --------------------------------------------------------------------------

PLANTED = dict(alpha=0.1, beta=0.05, l2w=1e-4, l2v=1e-4, loss="logistic")


def twin_logloss(s, d):
    import oracle
    yh = oracle.predict(float(s.w0), s.w, s.v, d["row_ptr"], d["col"], d["val"].astype(np.float64))
    return float(np.mean(ref.softplus(yh) - (d["y"] > 0) * yh))


@pytest.fixture(scope="module")
def planted():
    """The task, the start, and the twin's runs (computed once): l1w = 0.5 with l1v = 0, and l1v = 0.1 beside it."""
    train, test, info = fref.planted_task()
    n1 = int(train["col"].max()) + 1         # the model FM makes: dimension + 1
    assert n1 == 200
    init = (0.0, np.zeros(n1), np.random.default_rng(11).normal(0, 0.01, (4, n1)))
    twins = {}
    for l1w, l1v in ((0.5, 0.0), (0.5, 0.1)):
        s = fref.State(*init, 0.0, PLANTED["beta"])
        fref.epochs(s, train, 250, [None] * 20, PLANTED["alpha"], 0.0, PLANTED["l2w"], PLANTED["l2v"], fref.Rule("logistic", False, PLANTED["beta"], l1w, l1v))
        twins[(l1w, l1v)] = s
    return dict(train=train, test=test, info=info, noise=np.arange(20, 200), init=init, twins=twins)


@pytest.mark.parametrize("l1w,l1v", [(0.5, 0.0), (0.5, 0.1)])
def test_fm_learnwith_ftrl_on_a_planted_sparse_task(fmhip, planted, l1w, l1v):
    """FM(train, 4, maxIteration=20).learnWith(HipFTRL.run(...)): 200 binary features, 20 informative, 180 noise, 16 batches.  The
    GPU's test log-loss equals the twin's within rel 1e-5 and the share of noise w at exactly zero within the 1 % cap; what the
    twin shows is asserted of the GPU: with l1w = 0.5 more than half of the noise weights are exactly zero and no informative one
    is; with l1v = 0.1 (above the initial scale of V) EVERY factor row is zero, the informative ones too."""
    from sparkfm_amd import FM, DataSet
    train = DataSet.from_arrays(planted["train"], batch_rows=250).cache()
    test = DataSet.from_arrays(planted["test"]).cache()
    fm = FM(train, 4, maxIteration=20).learnWith(fmhip.HipFTRL.run(l1w=l1w, l1v=l1v, **PLANTED), init=planted["init"])
    s = planted["twins"][(l1w, l1v)]
    noise, info = planted["noise"], planted["info"]
    ll, ll_twin = fm.computeLogLoss(test), twin_logloss(s, planted["test"])
    share, share_twin = float((fm.w[noise] == 0).mean()), float((s.w[noise] == 0).mean())
    print("test log-loss %.6f (twin %.6f), noise w at zero %.4f (twin %.4f), informative w at zero %d (twin %d), v nonzero %d (twin %d)" % (
        ll, ll_twin, share, share_twin, (fm.w[info] == 0).sum(), (s.w[info] == 0).sum(), (fm.v != 0).sum(), (s.v != 0).sum()))
    assert ll == pytest.approx(ll_twin, rel=1e-5)
    assert abs(share - share_twin) <= fref.ZERO_CAP
    assert share_twin > 0.5 and share > 0.5
    assert (s.w[info] != 0).all() and (fm.w[info] != 0).all()
    assert ll_twin < np.log(2.0) - 0.1
    nz = fm.nonzeros()
    assert nz["w_nonzero"] == int((fm.w != 0).sum()) and nz["v_nonzero"] == int((fm.v != 0).sum())
    if l1v > 0:
        assert (s.v == 0).all() and nz["v_nonzero"] == 0 and nz["features_all_zero"] == int((fm.w == 0).sum())
    else:
        assert (s.v != 0).all() and nz["v_nonzero"] == 4 * 200
    train.unpersist()
    test.unpersist()
    fm.close()


# ---- 10. include/sparkfm.hpp ----------------------------------------------------------------------------------------------------

def test_cpp_hipftrl_matches_the_python_learner(fmhip, tmp_path):
    """tests/cpp_ftrl.cpp builds a small click dataset and a model from integer formulas, runs two HipFTRL epochs through
    include/sparkfm.hpp and prints every number as a hex float; the Python learner over the same formulas gives the same bits."""
    from sparkfm_amd import _build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_ftrl")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_ftrl.cpp"), "-L" + _build.LIBDIR, "-lfmhip",
                           "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    out = {}
    for line in r.stdout.decode().split("\n"):
        if line.strip():
            key, *vals = line.split()
            out[key] = [float.fromhex(x) for x in vals]
    n_rows, n1, k = 1000, 301, 8
    rows = []
    for r_ in range(n_rows):
        idx, val, s = [], [], 0.0
        for j in range(3 + r_ % 6):
            i = (r_ * 13 + j * 101 + (r_ * j) % 7) % n1
            if i in idx:
                continue
            x = 0.5 + ((r_ + j) % 4) / 8.0
            idx.append(i)
            val.append(x)
            s += x * ((i % 5) - 2) * 0.2
        rows.append((1.0 if s > 0.0 else 0.0, (idx, val)))
    ds = fmhip.DataSet.from_rows(rows, batch_rows=250).cache()
    fm = fmhip.FMModel(n1 - 1, k)
    fm.w0 = 0.1
    fm.w = [0.02 * ((i % 7) - 3) for i in range(n1)]
    fm.v = np.array([[0.01 * ((f * 7 + i * 3) % 11 - 5) for i in range(n1)] for f in range(k)])
    before = fm.computeLogLoss(ds)
    learner = fmhip.HipFTRL.run(alpha=0.1, beta=0.5, l1w=0.05, l1v=0.002, l2w=1e-4, l2v=1e-4, ftrl_init=0.1, loss="logistic")
    learner.learn(fm, ds)
    learner.learn(fm, ds)
    nz = fm.nonzeros()
    assert out["logloss"] == [before, fm.computeLogLoss(ds)] and out["logloss"][1] < out["logloss"][0]
    assert out["nonzeros"] == [nz["w_nonzero"], nz["v_nonzero"], nz["features_all_zero"]]
    assert out["w0"] == [fm.w0] and out["w"] == fm.w.tolist() and out["v"] == fm.v.reshape(-1, order="F").tolist()
    assert 0 < nz["w_nonzero"] < n1 or 0 < nz["v_nonzero"] < n1 * k          # the L1 left some of the model exactly zero, not all
    ds.unpersist()
    fm.close()
