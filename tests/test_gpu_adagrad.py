"""AdaGrad on every SGD training path (fmhip_model_set_optimizer, FMHIP_OPT_ADAGRAD): one step and epochs against the fp64
reference of train_ref.py (oracle.batch_grad + the rule in numpy), switches that must not change the result, the
accumulators' lifecycle, the data-parallel exchanges with thread ranks, and the public learners.

Every comparison against fp64 starts the accumulators above zero (initial_accumulator 0.1): with 0 the first step is
eta*sign(g), discontinuous where the true gradient is about zero.  0 appears only in bitwise GPU-against-GPU comparisons."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import train_ref as ref
from helpers import random_problem
from test_gpu_parity import TOL_G
from train_ref import DP_FRACTIONS, DP_ROWS, dp_init, dp_shard, make, rel, same

pytestmark = pytest.mark.gpu

EPS = 1e-10


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def L():
    from sparkfm_amd import _ffi
    return _ffi.load()


def set_opt(fm, opt="adagrad", eps=EPS, init=0.1):
    from sparkfm_amd import _ffi
    _ffi.check(L().fmhip_model_set_optimizer(fm.handle, _ffi.optimizer_code(opt), eps, init))


def get_state(fm):
    from sparkfm_amd import _ffi
    n1, k = fm.num_attribute + 1, fm.num_factor
    n0, nw, nv = C.c_double(), np.zeros(n1), np.zeros(n1 * k)
    _ffi.check(L().fmhip_model_get_optimizer_state(fm.handle, C.byref(n0), _ffi.ptr(nw), _ffi.ptr(nv)))
    return n0.value, nw, nv.reshape((k, n1), order="F")


def set_state(fm, n0, nw, nv):
    from sparkfm_amd import _ffi
    flat = np.ascontiguousarray(np.asarray(nv, np.float64).reshape(-1, order="F"))
    _ffi.check(L().fmhip_model_set_optimizer_state(fm.handle, n0, _ffi.ptr(np.ascontiguousarray(nw, np.float64)), _ffi.ptr(flat)))


def problem(seed, n_rows, n1, k, lo, hi, loss):
    a = random_problem(seed, n_rows, n1, k, lo, hi)
    if loss == "logistic":
        a["y"] = (np.random.default_rng(seed + 1).random(n_rows) < 0.4).astype(np.float64)
    return a


def rowtol(d_ref, floor_rel=1e-3):
    """TOL_G of test_gpu_parity.py on a per-feature basis: relative to the largest entry of the feature's column, floored by
    a thousandth of the largest anywhere (differences of sums that cancel)."""
    scale = max(np.abs(d_ref).max(), 1e-12)
    return TOL_G * np.maximum(np.abs(d_ref).max(axis=0), floor_rel * scale)


def check_step(fm, s0, s1, init, eta):
    """The GPU's step (fm's parameters and accumulators) against the reference step s0 -> s1 (fp64).  The change of every
    parameter is checked, within TOL_G of its feature's largest change, and the accumulator's growth likewise (2 x TOL_G: it
    is a square)."""
    n0, nw, nv = get_state(fm)
    f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)         # noqa: E731 — the device starts from the fp32 values
    dv_ref, dv = s1.v - s0.v, fm.v - f32(s0.v)
    assert (np.abs(dv - dv_ref) <= 2 * rowtol(dv_ref)[None, :] + 1.2e-7 * np.abs(s1.v)).all(), float(np.abs(dv - dv_ref).max())
    gv_ref, gv = s1.nv - init, nv - f32(init)
    assert (np.abs(gv - gv_ref) <= 2 * rowtol(gv_ref)[None, :] + 3e-7 * s1.nv).all(), float(np.abs(gv - gv_ref).max())
    dw_ref, dw = s1.w - s0.w, fm.w - f32(s0.w)
    assert (np.abs(dw - dw_ref) <= 2 * TOL_G * max(np.abs(dw_ref).max(), 1e-9) + 1.2e-7 * np.abs(s1.w)).all(), float(np.abs(dw - dw_ref).max())
    gw_ref, gw = s1.nw - init, nw - f32(init)
    assert (np.abs(gw - gw_ref) <= 2 * TOL_G * max(np.abs(gw_ref).max(), 1e-12) + 3e-7 * s1.nw).all(), float(np.abs(gw - gw_ref).max())
    assert fm.w0 - f32(s0.w0) == pytest.approx(s1.w0 - s0.w0, rel=2 * TOL_G, abs=1.2e-7 * abs(s1.w0) + 1e-9)
    assert n0 - f32(init) == pytest.approx(s1.n0 - init, rel=2 * TOL_G, abs=3e-7 * init)
    # it moved, by AdaGrad's steps: larger than SGD's eta*|g_hat| by about 1/sqrt(init) where g_hat is small
    assert np.abs(dv).max() > 1.5 * eta * np.sqrt((s1.nv - init).max())


# ---- 1. one step against the reference --------------------------------------------------------------------------------

# k -> (Kp, packed w slot?): 8 / 32 (Kp 32), 48 / 64 (Kp 64), 100 / 128 (Kp 128), 200 / 256 (Kp 256)
KS = [8, 32, 48, 64, 100, 128, 200, 256]


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("path", ["dense", "rows"])
def test_one_step_vs_reference(fmhip, k, loss, path):
    """fmhip_sgd_step under AdaGrad: V, w, w0 and the three accumulators.  dense: regv > 0 (the whole model moves, k_apply);
    rows: reg = 0 on a model far wider than the batch (k_apply_rows on the touched rows only — the others must not move)."""
    if path == "dense":
        a, regs, init = problem(40 + k, 400, 300, k, 1, 25, loss), (1e-3, 2e-3, 3e-3), 0.1
    else:
        a, regs, init = problem(60 + k, 150, 6000, k, 1, 12, loss), (0.0, 0.0, 0.0), 0.1
    eta = 0.05
    ds, fm = make(fmhip, a, batch_rows=0, loss=loss)
    set_opt(fm, init=init)
    s0 = ref.State(a["w0"], a["w"], a["v"], init)
    s1 = ref.step(s0.copy(), a["row_ptr"], a["col"], a["val"], a["y"], 0, len(a["y"]), eta, *regs, ref.Rule(loss, False, EPS))
    fmhip.HipSGD(eta=eta, reg0=regs[0], regw=regs[1], regv=regs[2], loss=loss, optimizer="adagrad", adagrad_init=init).step(fm, ds, 0)
    check_step(fm, s0, s1, init, eta)
    if path == "rows":
        untouched = np.setdiff1d(np.arange(a["n1"]), a["col"])
        assert len(untouched) > a["n1"] // 2
        _, nw, nv = get_state(fm)
        assert np.array_equal(fm.v[:, untouched], a["v"][:, untouched].astype(np.float32))
        assert (nv[:, untouched] == np.float32(init)).all() and (nw[untouched] == np.float32(init)).all()
    ds.unpersist()
    fm.close()


# ---- 2. epochs against the reference ----------------------------------------------------------------------------------

@pytest.mark.parametrize("k,loss,regs", [(32, "squared", (1e-3, 1e-3, 2e-3)), (20, "logistic", (1e-3, 1e-3, 2e-3)),
                                         (64, "squared", (0.0, 0.0, 0.0)), (130, "logistic", (0.0, 0.0, 0.0))])
def test_epochs_vs_reference(fmhip, k, loss, regs):
    """Two shuffled epochs of several batches (HipSGD.learn): relative L2 error 1e-5 (dp_cases.check's bound)."""
    n1 = 500 if regs[2] else 5000
    a = problem(7 + k, 900, n1, k, 2, 20, loss)
    ds, fm = make(fmhip, a, batch_rows=200, loss=loss)
    sgd = fmhip.HipSGD(eta=0.05, reg0=regs[0], regw=regs[1], regv=regs[2], shuffle_seed=3, loss=loss, optimizer="adagrad")
    orders = []
    for _ in range(2):
        orders.append(sgd.batch_order(ds.n_batches).tolist())
        sgd.learn(fm, ds)
    s = ref.epochs(ref.State(a["w0"], a["w"], a["v"], 0.1), a, 200, orders, 0.05, *regs, ref.Rule(loss, False, EPS))
    n0, nw, nv = get_state(fm)
    assert rel(fm.v, s.v) <= 1e-5 and rel(fm.w, s.w) <= 1e-5, (rel(fm.v, s.v), rel(fm.w, s.w))
    assert rel(nv, s.nv) <= 1e-5 and rel(nw, s.nw) <= 1e-5, (rel(nv, s.nv), rel(nw, s.nw))
    assert fm.w0 == pytest.approx(s.w0, rel=1e-5, abs=1e-6) and n0 == pytest.approx(s.n0, rel=1e-5)
    ds.unpersist()
    fm.close()


# ---- 3. switches that must not change AdaGrad's results ---------------------------------------------------------------

def train_bits(fmhip, a, regs, tune, init=0.0, epochs=2):
    from sparkfm_amd import _ffi
    ds, fm = make(fmhip, a, batch_rows=150)
    for key, val in tune.items():
        _ffi.check(L().fmhip_model_tune(fm.handle, _ffi.TUNE[key], val))
    set_opt(fm, init=init)
    sgd = fmhip.HipSGD(eta=0.05, reg0=regs[0], regw=regs[1], regv=regs[2], optimizer="adagrad", adagrad_init=init)
    for _ in range(epochs):
        sgd.learn(fm, ds)
    out = (fm.w0, fm.w.copy(), fm.v.copy()) + get_state(fm)
    ds.unpersist()
    fm.close()
    return out


@pytest.mark.parametrize("regs,n1", [((1e-3, 1e-3, 1e-3), 300), ((0.0, 0.0, 0.0), 4000)])
def test_fused_and_merged_switches_do_not_change_adagrad(fmhip, regs, n1):
    """FMHIP_TUNE_FUSED_UPDATE = 1 and FMHIP_TUNE_MERGED_FINISH = 0 / 1 only choose where an SGD update runs; under AdaGrad
    the update is its own launch whatever they say: bit-identical results (accumulators 0 at the start: GPU against GPU)."""
    a = problem(91, 600, n1, 32, 2, 20, "squared")
    base = train_bits(fmhip, a, regs, {})
    for tune in ({"FUSED_UPDATE": 1}, {"MERGED_FINISH": 0}, {"MERGED_FINISH": 1}, {"FUSED_UPDATE": 1, "MERGED_FINISH": 1}):
        assert same(base, train_bits(fmhip, a, regs, tune)), tune


# ---- 4. the accumulators' lifecycle -----------------------------------------------------------------------------------

def test_state_lifecycle(fmhip):
    from sparkfm_amd import _ffi
    a = problem(17, 500, 400, 24, 2, 20, "squared")
    regs = (1e-3, 1e-3, 2e-3)
    ds, fm = make(fmhip, a, batch_rows=200)
    n0 = C.c_double()
    assert L().fmhip_model_get_optimizer_state(fm.handle, C.byref(n0), None, None) == -1        # SGD: no state
    set_opt(fm, init=0.25)
    s = get_state(fm)
    assert s[0] == 0.25 and (s[1] == 0.25).all() and (s[2] == 0.25).all()
    sgd = fmhip.HipSGD(eta=0.05, reg0=regs[0], regw=regs[1], regv=regs[2], optimizer="adagrad", adagrad_init=0.25)
    sgd.learn(fm, ds)
    s1 = get_state(fm)
    assert (s1[2] > 0.25).any()
    set_opt(fm, init=0.25)                                        # the same settings again: a no-op that keeps the state
    assert same(s1, get_state(fm))
    set_opt(fm, init=0.5)                                         # other settings: a fresh state
    assert (get_state(fm)[2] == 0.5).all()
    set_opt(fm, eps=1e-8, init=0.5)
    assert (get_state(fm)[2] == 0.5).all()
    # get / set round trip (fp32 values go through fp64 exactly)
    sgd2 = fmhip.HipSGD(eta=0.05, reg0=regs[0], regw=regs[1], regv=regs[2], optimizer="adagrad", adagrad_eps=1e-8, adagrad_init=0.5)
    sgd2.learn(fm, ds)
    st = get_state(fm)
    set_state(fm, 1.5, np.full_like(st[1], 2.0), np.full_like(st[2], 3.0))
    t = get_state(fm)
    assert t[0] == 1.5 and (t[1] == 2.0).all() and (t[2] == 3.0).all()
    set_state(fm, *st)
    assert same(st, get_state(fm))
    bad = st[2].copy()
    bad[0, 0] = -1.0
    with pytest.raises(_ffi.FmhipError):
        set_state(fm, st[0], st[1], bad)
    bad[0, 0] = np.nan
    with pytest.raises(_ffi.FmhipError):
        set_state(fm, st[0], st[1], bad)
    # SGD frees the state and refuses the state calls
    set_opt(fm, "sgd")
    assert L().fmhip_model_get_optimizer_state(fm.handle, C.byref(n0), None, None) == -1
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("regs", [(1e-3, 1e-3, 2e-3), (0.0, 0.0, 0.0)])
def test_sgd_after_adagrad_trains_as_a_model_that_never_was(fmhip, regs):
    a = problem(23, 500, 3000, 16, 2, 20, "squared")
    outs = []
    for detour in (False, True):
        ds, fm = make(fmhip, a, batch_rows=200)
        if detour:
            set_opt(fm, init=0.1)
            set_opt(fm, "sgd")
        fmhip.HipSGD(eta=0.05, reg0=regs[0], regw=regs[1], regv=regs[2]).learn(fm, ds)
        outs.append((fm.w0, fm.w.copy(), fm.v.copy()))
        ds.unpersist()
        fm.close()
    assert same(outs[0], outs[1])


@pytest.mark.parametrize("k,regs", [(32, (1e-3, 1e-3, 2e-3)), (40, (0.0, 0.0, 0.0))])
def test_resume_is_bitwise(fmhip, k, regs):
    """Two epochs in a row == one epoch, then params + state copied into a FRESH model (set_params, set_optimizer, set_state),
    then the second epoch — bit for bit (accumulators started at 0: GPU against GPU)."""
    a = problem(29, 600, 2500, k, 2, 20, "squared")
    sgd = dict(eta=0.05, reg0=regs[0], regw=regs[1], regv=regs[2], optimizer="adagrad", adagrad_init=0.0)
    ds, fm = make(fmhip, a, batch_rows=200)
    fmhip.HipSGD(**sgd).learn(fm, ds)
    mid = (fm.w0, fm.w.copy(), fm.v.copy()) + get_state(fm)
    fmhip.HipSGD(**sgd).learn(fm, ds)
    straight = (fm.w0, fm.w.copy(), fm.v.copy()) + get_state(fm)
    fm.close()
    fm2 = fmhip.FMModel(a["n1"] - 1, k)
    fm2.w0, fm2.w, fm2.v = mid[0], mid[1], mid[2]
    set_opt(fm2, init=0.0)
    set_state(fm2, *mid[3:])
    fmhip.HipSGD(**sgd).learn(fm2, ds)
    assert same(straight, (fm2.w0, fm2.w.copy(), fm2.v.copy()) + get_state(fm2))
    ds.unpersist()
    fm2.close()


# ---- 5. data-parallel, thread ranks on one GPU ------------------------------------------------------------------------

def dp_run(world, exchange, shards, n1, k, br, epochs, regs, orders=None, init=0.1, setup=None):
    from sparkfm_amd import DataSet, FMModel
    from sparkfm_amd.distributed import HipDataParallelSGD, ThreadStagedComm, run_thread_ranks

    def rank_fn(r, group):
        ds = DataSet.from_arrays(shards[r], batch_rows=br, device=0).cache()
        fm = FMModel(n1 - 1, k, device=0)
        fm.w0, fm.w, fm.v = dp_init(n1, k)
        comm = ThreadStagedComm(fm, r, group)
        dp = HipDataParallelSGD(comm, eta=0.05, reg0=regs[0], regw=regs[1], regv=regs[2], exchange=exchange,
                                upper_fractions=DP_FRACTIONS[exchange], optimizer="adagrad", adagrad_init=init)
        out = {}
        try:
            dp.plan(fm, ds)
            for e in range(epochs):
                dp.learn(fm, ds, order=None if orders is None else orders[e])
            out = dict(w0=fm.w0, w=fm.w.copy(), v=fm.v.copy(), state=get_state(fm), rc=0)
        except Exception as ex:           # noqa: BLE001 — the refusals are what some cases test
            out = dict(rc=getattr(ex, "code", "?"), msg=str(ex))
        group.barrier()
        comm.close()
        ds.unpersist()
        fm.close(discard=True)
        return out

    return run_thread_ranks(world, rank_fn, timeout=300.0)


@pytest.mark.parametrize("world,exchange,shuffle", [(2, "dense", False), (8, "dense", False), (2, "pipelined", False), (2, "pipelined", True),
                                                    (8, "pipelined", True), (2, "touched", False), (8, "touched", False)])
def test_adagrad_data_parallel(fmhip, world, exchange, shuffle):
    """HipDataParallelSGD(optimizer="adagrad"): every replica (parameters AND accumulators) bitwise equal to rank 0's, and the
    fp64 reference over the global batches matched within rel-L2 1e-5.  The touched exchange runs without decay (its rows-only
    update is exact there); the others with it."""
    rows, n1_data, k, br, epochs = DP_ROWS[world], 800, 32, 250, 2
    n1 = 803 if exchange != "touched" else 4003
    regs = (0.0, 0.0, 0.0) if exchange == "touched" else (1e-3, 1e-3, 2e-3)
    shards = [dp_shard(4321, rows[r], r, rows, n1_data) for r in range(world)]
    steps = max((len(d["y"]) + br - 1) // br for d in shards)
    orders = [np.random.default_rng(e).permutation(steps).tolist() for e in range(epochs)] if shuffle else None
    res = dp_run(world, exchange, shards, n1, k, br, epochs, regs, orders)
    assert all(o["rc"] == 0 for o in res), [o.get("msg") for o in res]
    for r in range(1, world):
        assert same((res[0]["w0"], res[0]["w"], res[0]["v"]) + res[0]["state"], (res[r]["w0"], res[r]["w"], res[r]["v"]) + res[r]["state"]), r
    w0, w, v = dp_init(n1, k)
    s = ref.dp_epochs(ref.State(w0, w, v, 0.1), shards, br, orders or [None] * epochs, 0.05, *regs, ref.Rule(eps=EPS))
    assert rel(res[0]["v"], s.v) <= 1e-5 and rel(res[0]["w"], s.w) <= 1e-5, (rel(res[0]["v"], s.v), rel(res[0]["w"], s.w))
    assert rel(res[0]["state"][2], s.nv) <= 1e-5 and rel(res[0]["state"][1], s.nw) <= 1e-5
    assert abs(res[0]["w0"] - s.w0) <= 1e-5 * abs(s.w0) + 1e-6


@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("exchange,regs,code", [("sharded", (0.0, 0.0, 0.0), -5), ("touched", (0.0, 1e-3, 1e-3), -1)])
def test_adagrad_data_parallel_refusals(fmhip, world, exchange, regs, code):
    """The sharded exchange is refused under AdaGrad at the plan (FMHIP_ERR_UNSUPPORTED), the touched exchange with decay at
    the epoch — on every rank alike, nobody left inside a collective; the message names AdaGrad."""
    rows = DP_ROWS[world]
    shards = [dp_shard(99, rows[r], r, rows, 300) for r in range(world)]
    res = dp_run(world, exchange, shards, 303, 16, 250, 1, regs)
    assert [o["rc"] for o in res] == [code] * world, [o.get("msg") for o in res]
    assert all("AdaGrad" in o["msg"] for o in res), res[0]["msg"]


@pytest.mark.parametrize("world", [2, 8])
def test_adagrad_plan_agreement(fmhip, world):
    """Ranks with different optimizers, or the same optimizer with different eps: fmhip_dp_plan fails on every rank.  The
    sharded exchange set AFTER an AdaGrad plan is refused at the step on every rank.  An optimizer changed after the plan:
    fmhip_dp_epoch fails on every rank before its first collective (no hang)."""
    from sparkfm_amd import DataSet, FMModel, _ffi
    from sparkfm_amd.distributed import ThreadStagedComm, run_thread_ranks
    rows = DP_ROWS[world]
    shards = [dp_shard(98, rows[r], r, rows, 300) for r in range(world)]

    def rank_fn(r, group):
        ds = DataSet.from_arrays(shards[r], batch_rows=250, device=0).cache()
        fm = FMModel(302, 16, device=0)
        fm.w0, fm.w, fm.v = dp_init(303, 16)
        comm = ThreadStagedComm(fm, r, group)
        lib = L()
        fr = np.array([0.3])
        _ffi.check(lib.fmhip_dp_exchange(comm.handle, _ffi.EXCHANGE_DENSE))
        out = {}

        def plan():
            return lib.fmhip_dp_plan(fm.handle, ds.handle, comm.handle, 1, _ffi.ptr(fr), None)

        set_opt(fm, "adagrad" if r == 1 else "sgd")
        out["mixed_opt"] = plan()
        set_opt(fm, "adagrad", eps=1e-8 if r == world - 1 else EPS)
        out["mixed_eps"] = plan()
        set_opt(fm, "adagrad", eps=EPS)
        out["agreed"] = plan()
        _ffi.check(lib.fmhip_dp_exchange(comm.handle, _ffi.EXCHANGE_SHARDED))
        out["sharded_step"] = lib.fmhip_dp_step(fm.handle, ds.handle, 0 if ds.n_batches else -1, comm.handle, 0.05, 0.0, 0.0, 0.0)
        _ffi.check(lib.fmhip_dp_exchange(comm.handle, _ffi.EXCHANGE_DENSE))
        out["replan"] = plan()
        if r == 1:
            set_opt(fm, "adagrad", init=0.5)                       # behind the plan's back
        st = _ffi.Stats()
        out["epoch"] = lib.fmhip_dp_epoch(fm.handle, ds.handle, comm.handle, 0.05, 0.0, 0.0, 0.0, C.byref(st))
        group.barrier()
        comm.close()
        ds.unpersist()
        fm.close(discard=True)
        return out

    res = run_thread_ranks(world, rank_fn, timeout=120.0)
    assert [o["mixed_opt"] for o in res] == [-1] * world
    assert [o["mixed_eps"] for o in res] == [-1] * world
    assert [o["agreed"] for o in res] == [0] * world
    assert [o["sharded_step"] for o in res] == [-5] * world
    assert [o["replan"] for o in res] == [0] * world
    assert [o["epoch"] for o in res] == [-1] * world


PLAN_THEN_CHANGE = {        # field -> (the rule every rank plans under, what rank 1 then sets, what its refusal names)
    "loss": ({}, dict(loss=1), ["loss 0", "loss 1", "fmhip_model_set_loss"]),
    "pairing": ({}, dict(pairing=1), ["pairing 0", "pairing 1", "fmhip_model_set_pairing"]),
    "opt": ({}, dict(opt=("adagrad", EPS, 0.1)), ["optimizer 0", "optimizer 1", "fmhip_model_set_optimizer"]),
    "ada_eps": (dict(opt=("adagrad", EPS, 0.1)), dict(opt=("adagrad", 1e-8, 0.1)), ["eps 1e-10", "eps 1e-08", "fmhip_model_set_optimizer"]),
    "ada_init": (dict(opt=("adagrad", EPS, 0.1)), dict(opt=("adagrad", EPS, 0.5)),
                 ["initial accumulator 0.1", "initial accumulator 0.5", "fmhip_model_set_optimizer"]),
}


@pytest.mark.parametrize("field", sorted(PLAN_THEN_CHANGE))
def test_rule_changed_after_the_plan_is_that_ranks_failure(fmhip, field):
    """Two ranks plan under one rule, then rank 1 alone changes one of its five fields and both take fmhip_dp_step_at(0):
    rank 1 is refused (FMHIP_ERR_INVALID naming the field, the planned and the present value, the setter, and the way out) but
    has taken the step's collectives with a zero contribution — rank 0's step completes, and both ranks issued the same
    (kind, count) sequence."""
    from sparkfm_amd import DataSet, FMModel, _ffi
    from sparkfm_amd.distributed import ThreadStagedComm, run_thread_ranks
    base, change, names = PLAN_THEN_CHANGE[field]
    rows = [64, 64]
    shards = [dp_shard(97, rows[r], r, rows, 100) for r in range(2)]

    def rank_fn(r, group):
        ds = DataSet.from_arrays(shards[r], batch_rows=32, device=0).cache()
        fm = FMModel(100, 8, device=0)
        fm.w0, fm.w, fm.v = dp_init(101, 8)
        comm = ThreadStagedComm(fm, r, group)
        lib = L()

        def set_fields(loss=None, pairing=None, opt=None):
            if loss is not None:
                _ffi.check(lib.fmhip_model_set_loss(fm.handle, loss))
            if pairing is not None:
                _ffi.check(lib.fmhip_model_set_pairing(fm.handle, pairing))
            if opt is not None:
                set_opt(fm, *opt)

        set_fields(**base)
        fr = np.array([0.3])
        _ffi.check(lib.fmhip_dp_plan(fm.handle, ds.handle, comm.handle, 1, _ffi.ptr(fr), None))
        if r == 1:
            set_fields(**change)
        before = len(comm.calls)
        rc = lib.fmhip_dp_step_at(fm.handle, ds.handle, 0, comm.handle, 0.05, 0.0, 0.0, 0.0)
        out = dict(rc=rc, msg=lib.fmhip_last_error().decode() if rc else "", calls=comm.calls[before:])
        group.barrier()
        comm.close()
        ds.unpersist()
        fm.close(discard=True)
        return out

    res = run_thread_ranks(2, rank_fn, timeout=60.0)
    assert res[0]["rc"] == 0, res[0]["msg"]
    assert res[1]["rc"] == -1
    for name in names + ["call fmhip_dp_plan again (every rank)", "contributed zeros"]:
        assert name in res[1]["msg"], (name, res[1]["msg"])
    assert res[0]["calls"] == res[1]["calls"] and len(res[0]["calls"]) >= 2


# ---- 6. through the public flow ----------------------------------------------------------------------------------------

def test_fm_learnwith_adagrad_lowers_rmse_and_logloss(fmhip):
    """FM(ds, k).learnWith(HipSGD.run(optimizer="adagrad")) lowers the training RMSE; with loss="logistic" on a small
    Criteo-shaped set (power-law feature frequencies, click labels) it lowers the log-loss."""
    from sparkfm_amd import FM, DataSet, synth
    d = synth.make_zipf(seed=5, n_rows=3000, n_features=4000, nnz_lo=5, nnz_hi=30, zipf_s=1.05)
    ds = DataSet.from_arrays(d, batch_rows=500, device=0).cache()
    fm0 = FM(ds, 16, maxIteration=0).learnWith(fmhip.HipSGD.run(eta=0.05, optimizer="adagrad"))
    r0 = fm0.computeRMSE(ds)
    fm = FM(ds, 16, maxIteration=3).learnWith(fmhip.HipSGD.run(eta=0.05, optimizer="adagrad"))
    assert fm.computeRMSE(ds) < 0.97 * r0
    dc = dict(d, y=(d["y"] > np.quantile(d["y"], 0.75)).astype(np.float32))      # ~25 % clicks
    dsc = DataSet.from_arrays(dc, batch_rows=500, device=0).cache()
    fmc0 = FM(dsc, 16, maxIteration=0).learnWith(fmhip.HipSGD.run(eta=0.05, loss="logistic", optimizer="adagrad"))
    l0 = fmc0.computeLogLoss(dsc)
    fmc = FM(dsc, 16, maxIteration=3).learnWith(fmhip.HipSGD.run(eta=0.05, loss="logistic", optimizer="adagrad"))
    assert fmc.computeLogLoss(dsc) < 0.98 * l0
    for m in (fm0, fm, fmc0, fmc):
        m.close()
    ds.unpersist()
    dsc.unpersist()


def test_hip_data_parallel_sgd_adagrad_lowers_rmse(fmhip):
    from sparkfm_amd import DataSet, FMModel
    from sparkfm_amd.distributed import HipDataParallelSGD, ThreadStagedComm, run_thread_ranks
    rows = [800, 700]
    shards = [dp_shard(55, rows[r], r, rows, 600) for r in range(2)]

    def rank_fn(r, group):
        ds = DataSet.from_arrays(shards[r], batch_rows=200, device=0).cache()
        fm = FMModel(602, 16, device=0)
        fm.w0, fm.w, fm.v = dp_init(603, 16)
        comm = ThreadStagedComm(fm, r, group)
        dp = HipDataParallelSGD(comm, eta=0.05, optimizer="adagrad", upper_fractions=(0.3,))
        before = fm.computeRMSE(ds)
        for _ in range(3):
            dp.learn(fm, ds)
        after = fm.computeRMSE(ds)
        group.barrier()
        comm.close()
        ds.unpersist()
        fm.close(discard=True)
        return before, after

    for before, after in run_thread_ranks(2, rank_fn, timeout=300.0):
        assert after < 0.9 * before, (before, after)


def test_cpp_hipsgd_adagrad(fmhip, tmp_path):
    """include/sparkfm.hpp's HipSGD with FMHIP_OPT_ADAGRAD: tests/cpp_adagrad.cpp fits a small model and reports the RMSE
    before and after; it must fall, and an SGD fit must differ from the AdaGrad one."""
    from sparkfm_amd import _build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_adagrad")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_adagrad.cpp"), "-L" + _build.LIBDIR, "-lfmhip",
                           "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    vals = dict(line.split() for line in r.stdout.decode().split("\n") if line.strip())
    assert float(vals["adagrad_after"]) < 0.9 * float(vals["before"]), vals
    assert float(vals["adagrad_after"]) != float(vals["sgd_after"]), vals
