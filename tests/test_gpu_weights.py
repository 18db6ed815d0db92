"""Per-row example weights on the device (include/fmhip_weights.h): every SGD training path against the fp64 twin of
weight_ref.py, the bitwise properties of the rule (power-of-two scaling, zero-weight rows), the refusals, fmhip_weighted_scores,
and include/sparkfm.hpp.

Weights are drawn from {0, 0.25, 1, 3.5} with about a fifth of the rows at 0 (weight_ref.draw_weights).  Tolerances: TOL_G of
test_gpu_parity.py per feature in the form of test_gpu_adagrad.check_step for one step, rel-L2 1e-5 (dp_cases.check) for
trajectories, rel 1e-5 (test_gpu_logistic.test_logloss_vs_numpy) for the scores."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import weight_ref as wref
from helpers import random_problem
from test_gpu_adagrad import EPS, check_step as check_adagrad_step, rowtol, set_opt
from test_gpu_parity import TOL_G
from train_ref import DP_FRACTIONS, DP_ROWS, dp_init, dp_shard, rel, same

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


def problem(seed, n_rows, n1, k, lo, hi, loss):
    a = random_problem(seed, n_rows, n1, k, lo, hi)
    if loss == "logistic":
        a["y"] = (np.random.default_rng(seed + 1).random(n_rows) < 0.4).astype(np.float64)
    a["c"] = wref.draw_weights(seed + 2, n_rows)
    return a


def make(fmhip, a, batch_rows=0, weights="c", y=None, scoring=False, stream=None):
    """-> (cached DataSet carrying a[weights] (None: unweighted), FMModel at the problem's parameters)."""
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"] if y is None else y, batch_rows=batch_rows, scoring=scoring,
                       weights=None if weights is None else (a[weights] if isinstance(weights, str) else weights)).cache()
    fm = fmhip.FMModel(a["n1"] - 1, a["k"], stream=stream)
    fm.w0, fm.w, fm.v = a["w0"], a["w"], a["v"]
    return ds, fm


def params(fm):
    return fm.w0, fm.w.copy(), fm.v.copy()


def check_step(fm, s0, s1):
    """The GPU's step against the twin's s0 -> s1: the change of every parameter within TOL_G of its feature's largest change —
    the form and constants of test_gpu_adagrad.check_step, without the accumulators plain SGD does not have."""
    f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)         # noqa: E731 — the device starts from the fp32 values
    dv_ref, dv = s1.v - s0.v, fm.v - f32(s0.v)
    assert (np.abs(dv - dv_ref) <= 2 * rowtol(dv_ref)[None, :] + 1.2e-7 * np.abs(s1.v)).all(), float(np.abs(dv - dv_ref).max())
    dw_ref, dw = s1.w - s0.w, fm.w - f32(s0.w)
    assert (np.abs(dw - dw_ref) <= 2 * TOL_G * max(np.abs(dw_ref).max(), 1e-9) + 1.2e-7 * np.abs(s1.w)).all(), float(np.abs(dw - dw_ref).max())
    assert fm.w0 - f32(s0.w0) == pytest.approx(s1.w0 - s0.w0, rel=2 * TOL_G, abs=1.2e-7 * abs(s1.w0) + 1e-9)
    assert np.abs(dv).max() > 1e-5                     # it moved


# ---- 1. one step against the twin -----------------------------------------------------------------------------------------

# k -> (Kp, packed w slot?): 8 / 32 (Kp 32), 48 / 64 (Kp 64), 100 / 128 (Kp 128), 200 / 256 (Kp 256)
KS = [8, 32, 48, 64, 100, 128, 200, 256]


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("path", ["dense", "rows"])
def test_one_step_vs_twin(fmhip, k, loss, path):
    """fmhip_sgd_step on a weighted dataset: V, w, w0.  dense: all three reg > 0 (the whole model moves); rows: reg = 0 on a model
    far wider than the batch (the rows-only update — the untouched rows must keep their bits).  The step's statistics are those
    of the weighted residual."""
    if path == "dense":
        a, regs = problem(140 + k, 400, 300, k, 1, 25, loss), (1e-3, 2e-3, 3e-3)
    else:
        a, regs = problem(160 + k, 150, 6000, k, 1, 12, loss), (0.0, 0.0, 0.0)
    eta, n = 0.05, len(a["y"])
    ds, fm = make(fmhip, a)
    dw = ds.deviceWeights()
    assert dw["weighted"] and np.array_equal(dw["weights"], a["c"]) and dw["sum"] == a["c"].sum() and 0.1 < (a["c"] == 0).mean() < 0.3
    rule = wref.Rule(loss, False, None)
    s0 = wref.State(a["w0"], a["w"], a["v"])
    e = wref.pseudo_targets(s0, a["row_ptr"], a["col"], a["val"], a["y"], a["c"], rule)[1]
    s1 = wref.step(s0.copy(), a["row_ptr"], a["col"], a["val"], a["y"], a["c"], 0, n, eta, *regs, rule)
    st = fmhip.HipSGD(eta=eta, reg0=regs[0], regw=regs[1], regv=regs[2], loss=loss).step(fm, ds, 0)
    check_step(fm, s0, s1)
    assert st["rows"] == n and st["nonfinite"] == 0
    assert st["sse"] == pytest.approx((e * e).sum(), rel=1e-5) and st["sum_e"] == pytest.approx(e.sum(), rel=1e-5, abs=1e-4)
    if path == "rows":
        untouched = np.setdiff1d(np.arange(a["n1"]), a["col"])
        assert len(untouched) > a["n1"] // 2
        assert np.array_equal(fm.v[:, untouched], a["v"][:, untouched].astype(np.float32))
        assert np.array_equal(fm.w[untouched], a["w"][untouched].astype(np.float32))
    ds.unpersist()
    fm.close()


# ---- 2. epochs against the twin ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,loss,regs,n1", [(32, "squared", (1e-3, 1e-3, 2e-3), 500), (20, "logistic", (1e-3, 1e-3, 2e-3), 500),
                                            (64, "squared", (0.0, 0.0, 0.0), 5000), (130, "logistic", (0.0, 0.0, 0.0), 5000),
                                            (64, "logistic", (1e-3, 1e-3, 2e-3), 20000)])
def test_epochs_vs_twin(fmhip, k, loss, regs, n1):
    """Two shuffled epochs, 900 rows in batches of 200 (the last one short): relative L2 error 1e-5 on v and w (dp_cases.check's
    bound).  The last case is a wide model with decay: a batch touches a few hundred of 20000 rows, the rows-only update with
    lazy weight decay."""
    a = problem(107 + k, 900, n1, k, 2, 20 if n1 < 20000 else 10, loss)
    ds, fm = make(fmhip, a, batch_rows=200)
    sgd = fmhip.HipSGD(eta=0.05, reg0=regs[0], regw=regs[1], regv=regs[2], shuffle_seed=3, loss=loss)
    orders = []
    for _ in range(2):
        orders.append(sgd.batch_order(ds.n_batches).tolist())
        sgd.learn(fm, ds)
    assert ds.n_batches == 5 and sgd.last_stats["rows"] == 900
    s = wref.epochs(wref.State(a["w0"], a["w"], a["v"]), a, a["c"], 200, orders, 0.05, *regs, wref.Rule(loss, False, None))
    assert rel(fm.v, s.v) <= 1e-5 and rel(fm.w, s.w) <= 1e-5, (rel(fm.v, s.v), rel(fm.w, s.w))
    assert fm.w0 == pytest.approx(s.w0, rel=1e-5, abs=1e-6)
    assert np.abs(fm.w - a["w"]).max() > 1e-4                # it moved
    ds.unpersist()
    fm.close()


# ---- 3. weights 2c, eta / 2, 2 reg: the same bits ------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k,n1,regs", [(8, 300, (1e-3, 2e-3, 3e-3)), (48, 300, (1e-3, 2e-3, 3e-3)), (100, 6000, (0.0, 1e-3, 2e-3)),
                                       (200, 6000, (0.0, 0.0, 0.0))])
def test_doubled_weights_halved_step_give_the_same_bits(fmhip, k, n1, regs, loss):
    """GPU against GPU, plain SGD: theta - (eta/2) (2 g / |B| + 2 reg theta) is theta - eta (g / |B| + reg theta) in every bit —
    doubling is exact in fp32 (nothing here is near the denormals), through the finish, the backward, the fixups and both
    updates (dense, and rows-only with lazy decay: 1 - eta reg is the same number).  The first step's sse is exactly 4 x.
    Packed rows only (k < Kp): where a P row has no spare slot the residual's 32 bits ride in the low mantissa bits of the row's
    first floats (kEInP, fm_device.h), a nudge of <= 2 ulp that depends on e's exponent bits, so there P(2e) is 2 P(e) only to
    2 ulp — by design, and covered against the twin in the tests above (measured, two epochs at k = 32 / 64 / 128: 89 of 9600,
    156 of 384000, 123 of 768000 entries of v differ, by at most 3.4e-8 of the largest; k = 8: none)."""
    a = problem(207 + k, 600, n1, k, 2, 20, loss)
    outs, sses = [], []
    for scale in (1.0, 2.0):
        ds, fm = make(fmhip, a, batch_rows=250, weights=a["c"] * scale)
        sgd = fmhip.HipSGD(eta=0.0625 / scale, reg0=regs[0] * scale, regw=regs[1] * scale, regv=regs[2] * scale, loss=loss)
        sses.append(sgd.step(fm, ds, 0)["sse"])
        for b in (1, 2, 0):
            sgd.step(fm, ds, b)
        sgd.learn(fm, ds)
        outs.append(params(fm))
        ds.unpersist()
        fm.close()
    assert same(outs[0], outs[1])
    assert sses[0] > 0 and sses[1] == 4.0 * sses[0]
    assert np.abs(outs[0][2] - a["v"]).max() > 1e-4            # it moved


# ---- 4. rows of weight 0 do not exist -------------------------------------------------------------------------------------

@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k,n1,regs", [(32, 300, (1e-3, 2e-3, 3e-3)), (8, 6000, (0.0, 0.0, 0.0)), (128, 6000, (0.0, 1e-3, 1e-3))])
def test_labels_of_zero_weight_rows_change_no_bit(fmhip, k, n1, regs, loss):
    """Three steps; then the same with only the labels of the zero-weight rows changed (sign flipped, moved far away): every
    parameter keeps its bits — their residual is +0 whatever the loss makes of them, in the row's P bits too (k = Kp)."""
    a = problem(307 + k, 500, n1, k, 2, 20, loss)
    zero = a["c"] == 0
    assert 50 < zero.sum() < 200
    y2 = a["y"].copy()
    y2[zero] = np.where(y2[zero] > 0, -50.0, 77.0)
    outs = []
    for y in (a["y"], y2):
        ds, fm = make(fmhip, a, batch_rows=200, y=y)
        sgd = fmhip.HipSGD(eta=0.05, reg0=regs[0], regw=regs[1], regv=regs[2], loss=loss)
        stats = [sgd.step(fm, ds, b) for b in (0, 1, 2)]
        outs.append(params(fm) + tuple(s["sse"] for s in stats) + tuple(s["sum_e"] for s in stats))
        ds.unpersist()
        fm.close()
    assert same(outs[0], outs[1])
    assert np.abs(outs[0][2] - a["v"]).max() > 1e-4


# ---- 5. the other rules: pairs with per-pair weights, AdaGrad ---------------------------------------------------------------

@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k", [32, 100])
def test_weighted_pairs_vs_twin(fmhip, k, loss):
    """HipSGD(pairs=True) on a dataset whose pairs carry weights (both rows of pair j hold c_j, as DataSet.from_pairs writes them):
    one step against the twin; the pair's residuals sum to exactly zero (sum_e == 0.0, w0 moves by reg0 only); row 2j+1's stored
    weight, replaced by garbage in the array handed to fmhip_dataset_create_weighted, changes no bit."""
    a = problem(407 + k, 400, 300, k, 1, 25, loss)
    cp = np.repeat(wref.draw_weights(5 + k, 200), 2)
    regs, eta = (1e-3, 2e-3, 3e-3), 0.05
    rule = wref.Rule(loss, True, None)
    s0 = wref.State(a["w0"], a["w"], a["v"])
    e = wref.pseudo_targets(s0, a["row_ptr"], a["col"], a["val"], a["y"], cp, rule)[1]
    assert np.array_equal(e[0::2], -e[1::2]) and np.abs(e).max() > 0.1
    s1 = wref.step(s0.copy(), a["row_ptr"], a["col"], a["val"], a["y"], cp, 0, 400, eta, *regs, rule)
    garbage = cp.copy()
    garbage[1::2] = np.random.default_rng(9).choice([0.0, 1e30, 7.5, 1e-30], 200)
    outs = []
    for c in (cp, garbage):
        ds, fm = make(fmhip, a, weights=c)
        st = fmhip.HipSGD(eta=eta, reg0=regs[0], regw=regs[1], regv=regs[2], loss=loss, pairs=True).step(fm, ds, 0)
        assert st["sum_e"] == 0.0 and st["sse"] == pytest.approx((e * e).sum(), rel=1e-5)
        check_step(fm, s0, s1)
        outs.append(params(fm))
        ds.unpersist()
        fm.close()
    assert same(outs[0], outs[1])


@pytest.mark.parametrize("k,loss,path", [(32, "squared", "dense"), (100, "logistic", "dense"), (32, "logistic", "rows"), (100, "squared", "rows")])
def test_weighted_adagrad_vs_twin(fmhip, k, loss, path):
    """AdaGrad takes the weighted g_hat as it takes any other: one step against the twin, parameters and accumulators
    (test_gpu_adagrad.check_step itself)."""
    if path == "dense":
        a, regs = problem(440 + k, 400, 300, k, 1, 25, loss), (1e-3, 2e-3, 3e-3)
    else:
        a, regs = problem(460 + k, 150, 6000, k, 1, 12, loss), (0.0, 0.0, 0.0)
    eta, init = 0.05, 0.1
    ds, fm = make(fmhip, a)
    from sparkfm_amd import _ffi
    _ffi.check(L().fmhip_model_set_loss(fm.handle, _ffi.loss_code(loss)))
    set_opt(fm, init=init)
    s0 = wref.State(a["w0"], a["w"], a["v"], init)
    s1 = wref.step(s0.copy(), a["row_ptr"], a["col"], a["val"], a["y"], a["c"], 0, len(a["y"]), eta, *regs, wref.Rule(loss, False, EPS))
    fmhip.HipSGD(eta=eta, reg0=regs[0], regw=regs[1], regv=regs[2], loss=loss, optimizer="adagrad", adagrad_init=init).step(fm, ds, 0)
    check_adagrad_step(fm, s0, s1, init, eta)
    ds.unpersist()
    fm.close()


# ---- 6. data parallel, thread ranks on one GPU ----------------------------------------------------------------------------------

def weighted_shards(world, seed, n1_data, binary, only=None):
    rows = DP_ROWS[world]
    shards = [dp_shard(seed, rows[r], r, rows, n1_data, binary=binary) for r in range(world)]
    return [dict(d, weights=wref.draw_weights(seed + 10 + r, rows[r])) if only is None or r in only else d for r, d in enumerate(shards)]


@pytest.mark.parametrize("world,exchange,loss", [(2, "dense", "squared"), (2, "sharded", "squared"), (2, "touched", "logistic"), (8, "dense", "logistic")])
def test_weighted_data_parallel(fmhip, world, exchange, loss):
    """HipDataParallelSGD over weighted shards (train_ref.DP_ROWS: world 8 has an empty rank): replicas bit-identical, the twin
    over the global batches — |B| their ROW count — matched within rel-L2 1e-5."""
    from sparkfm_amd import DataSet, FMModel
    from sparkfm_amd.distributed import HipDataParallelSGD, ThreadStagedComm, run_thread_ranks
    n1, k, br, n_epochs = 803, 32, 250, 2
    eta, regw, regv = 0.1, 1e-3, 1e-3
    shards = weighted_shards(world, 4321, 800, loss == "logistic")

    def rank_fn(r, group):
        ds = DataSet.from_arrays(shards[r], batch_rows=br, device=0).cache()
        assert ds.deviceWeights()["weighted"]
        fm = FMModel(n1 - 1, k, device=0)
        fm.w0, fm.w, fm.v = dp_init(n1, k)
        comm = ThreadStagedComm(fm, r, group)
        dp = HipDataParallelSGD(comm, eta=eta, regw=regw, regv=regv, exchange=exchange, upper_fractions=DP_FRACTIONS[exchange], loss=loss)
        dp.plan(fm, ds)
        for _ in range(n_epochs):
            dp.learn(fm, ds)
        out = dict(w0=fm.w0, w=fm.w.copy(), v=fm.v.copy())
        group.barrier()
        comm.close()
        ds.unpersist()
        fm.close(discard=True)
        return out

    res = run_thread_ranks(world, rank_fn, timeout=300.0)
    for r in range(1, world):
        assert np.array_equal(res[0]["v"], res[r]["v"]) and np.array_equal(res[0]["w"], res[r]["w"]) and res[0]["w0"] == res[r]["w0"], r
    s = wref.dp_epochs(wref.State(*dp_init(n1, k)), shards, br, [None] * n_epochs, eta, 0.0, regw, regv, wref.Rule(loss, False, None))
    assert rel(res[0]["v"], s.v) <= 1e-5 and rel(res[0]["w"], s.w) <= 1e-5, (rel(res[0]["v"], s.v), rel(res[0]["w"], s.w))
    assert abs(res[0]["w0"] - s.w0) <= 1e-5 * abs(s.w0) + 1e-6
    assert np.abs(res[0]["w"] - dp_init(n1, k)[1]).max() > 1e-3


def test_pipelined_exchange_refuses_weights_on_every_rank(fmhip):
    """Only rank 1's shard is weighted: fmhip_dp_plan under the pipelined exchange returns FMHIP_ERR_UNSUPPORTED on BOTH ranks
    (the flag travels in the plan's max-reduce), both ranks issued the same collectives, and nobody is left inside one: a dense
    plan and an epoch right after complete on both.  Without any weighted shard the pipelined plan passes."""
    from sparkfm_amd import DataSet, FMModel, _ffi
    from sparkfm_amd.distributed import HipDataParallelSGD, ThreadStagedComm, run_thread_ranks
    mixed, plain = weighted_shards(2, 99, 300, False, only=(1,)), weighted_shards(2, 99, 300, False, only=())

    def rank_fn(r, group):
        fm = FMModel(302, 16, device=0)
        fm.w0, fm.w, fm.v = dp_init(303, 16)
        before = params(fm)
        comm = ThreadStagedComm(fm, r, group)
        out = {}

        def plan(ds, **kw):
            n = len(comm.calls)
            try:
                HipDataParallelSGD(comm, eta=0.1, **kw).plan(fm, ds)
                return 0, "", comm.calls[n:]
            except _ffi.FmhipError as ex:
                return ex.code, str(ex), comm.calls[n:]
        ds = DataSet.from_arrays(mixed[r], batch_rows=250, device=0).cache()
        dsp = DataSet.from_arrays(plain[r], batch_rows=250, device=0).cache()
        assert ds.deviceWeights()["weighted"] == (r == 1)
        out["pipelined"] = plan(ds, exchange="pipelined", upper_fractions=(0.1, 0.3, 0.6))
        fm._device_updated()
        out["unchanged"] = same(before, params(fm))
        out["pipelined_plain"] = plan(dsp, exchange="pipelined", upper_fractions=(0.1, 0.3, 0.6))[0]
        dense = HipDataParallelSGD(comm, eta=0.1, exchange="dense", upper_fractions=(0.3,))
        dense.plan(fm, ds)
        dense.learn(fm, ds)
        out["v"] = fm.v.copy()
        group.barrier()
        comm.close()
        ds.unpersist()
        dsp.unpersist()
        fm.close(discard=True)
        return out

    res = run_thread_ranks(2, rank_fn, timeout=120.0)
    for o in res:
        assert o["pipelined"][0] == -5 and "pipelined" in o["pipelined"][1] and "weight" in o["pipelined"][1], o["pipelined"]
        assert o["unchanged"] and o["pipelined_plain"] == 0
    assert res[0]["pipelined"][2] == res[1]["pipelined"][2] and len(res[0]["pipelined"][2]) >= 1
    assert np.array_equal(res[0]["v"], res[1]["v"]) and np.abs(res[0]["v"] - dp_init(303, 16)[2]).max() > 1e-4


def test_host_staged_data_parallel_sgd_trains_weighted(fmhip):
    """DataParallelSGD's host-staged engine goes through fmhip_step_compute / fmhip_step_forward, so it trains a weighted dataset
    unchanged: one epoch (a single rank, no process group) against the twin, whole-batch and feature-interval backward."""
    import torch
    from sparkfm_amd.distributed import DataParallelSGD, HipEngine, torch_stream_handle
    a = problem(601, 600, 400, 24, 2, 20, "logistic")
    s = wref.epochs(wref.State(a["w0"], a["w"], a["v"]), a, a["c"], 200, [None], 0.05, 0.0, 1e-3, 1e-3, wref.Rule("logistic", False, None))
    ds, fm = make(fmhip, a, batch_rows=200, stream=torch_stream_handle(0))
    dp = DataParallelSGD(eta=0.05, regw=1e-3, regv=1e-3, loss="logistic")
    dp.learn(fm, ds)
    torch.cuda.synchronize()
    dp.engine(fm, ds).close()
    assert rel(fm.v, s.v) <= 1e-5 and rel(fm.w, s.w) <= 1e-5, (rel(fm.v, s.v), rel(fm.w, s.w))
    # the engine's pieces: forward, then the backward in two feature intervals
    fm2 = fmhip.FMModel(a["n1"] - 1, a["k"], stream=torch_stream_handle(0))
    fm2.w0, fm2.w, fm2.v = a["w0"], a["w"], a["v"]
    eng = HipEngine(fm2, ds)
    eng.set_rule(DataParallelSGD(loss="logistic").rule)
    for j in range(3):
        eng.forward(j)
        eng.backward(j, 150, a["n1"], False)
        eng.backward(j, 0, 150, True)
        eng.apply(0.05, 0.0, 1e-3, 1e-3)
    torch.cuda.synchronize()
    assert rel(fm2.v, s.v) <= 1e-5 and rel(fm2.w, s.w) <= 1e-5
    eng.close()
    ds.unpersist()
    fm.close()
    fm2.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------

def test_als_and_the_two_pass_forward_refuse_a_weighted_dataset(fmhip):
    """FMHIP_ERR_UNSUPPORTED, the message names the weights, the model keeps its bits; the same rows without weights pass."""
    from sparkfm_amd import _ffi
    a = problem(701, 400, 200, 16, 1, 20, "squared")
    ds, fm = make(fmhip, a)
    before = params(fm)
    assert L().fmhip_als_epoch(fm.handle, ds.handle, 0.0, 0.0, 10.0) == -5
    assert b"ALS" in L().fmhip_last_error() and b"weight" in L().fmhip_last_error()
    _ffi.check(L().fmhip_dataset_partition_rows(ds.handle, 100))
    for pass_ in (0, 1):
        assert L().fmhip_step_forward_pass(fm.handle, ds.handle, 0, pass_) == -5
        assert b"two-pass" in L().fmhip_last_error() and b"weight" in L().fmhip_last_error()
    fm._device_updated()
    assert same(before, params(fm))
    assert L().fmhip_sgd_step(fm.handle, ds.handle, 0, 0.05, 0.0, 0.0, 0.0, None) == 0       # ... and it trains
    ds.unpersist()
    fm.close()
    ds, fm = make(fmhip, a, weights=None)
    assert not ds.deviceWeights()["weighted"] and ds.deviceWeights()["sum"] == 400.0 and (ds.deviceWeights()["weights"] == 1.0).all()
    _ffi.check(L().fmhip_dataset_partition_rows(ds.handle, 100))
    for pass_ in (0, 1):
        assert L().fmhip_step_forward_pass(fm.handle, ds.handle, 0, pass_) == 0
    assert L().fmhip_als_epoch(fm.handle, ds.handle, 0.0, 0.0, 10.0) == 0
    res = _ffi.WeightedResult()
    assert L().fmhip_weighted_scores(fm.handle, ds.handle, C.byref(res)) == -1 and b"no example weights" in L().fmhip_last_error()
    ds.unpersist()
    fm.close()


# ---- 8. fmhip_weighted_scores ------------------------------------------------------------------------------------------------

def check_scores(fm, ds, y, c):
    got = fm.weightedScores(ds)
    want = wref.weighted_scores(fm.predict(ds), y, c)
    assert got["rows"] == len(y) and got["nonfinite"] == 0
    assert got["sum_w"] == np.asarray(c, np.float32).astype(np.float64).sum()
    for key in ("rmse", "mae", "logloss"):
        assert np.isfinite(got[key]) and got[key] == pytest.approx(want[key], rel=1e-5), (key, got[key], want[key])
    assert fm.computeWeightedRMSE(ds) == got["rmse"] and fm.computeWeightedLogLoss(ds) == got["logloss"]
    return got


def test_weighted_scores_vs_numpy(fmhip):
    """Against fp64 numpy over fm.predict, rel 1e-5 (test_gpu_logistic.test_logloss_vs_numpy's bound): on a training dataset of
    several batches and on a scoring=True dataset, labels {-1, +1}
    with an empty row; saturated margins stay finite; sum c == 0 gives NaN ratios and FMHIP_OK; two threads scoring one model get
    the bits of a lone caller; fmhip_rmse and fmhip_logloss ignore the weights bit for bit."""
    a = problem(801, 1500, 300, 24, 0, 30, "squared")
    a["y"] = np.where(np.random.default_rng(4).random(1500) < 0.4, 1.0, -1.0)
    ds, fm = make(fmhip, a, batch_rows=400)
    dss, _ = make(fmhip, a, scoring=True)
    plain, _ = make(fmhip, a, batch_rows=400, weights=None)
    for w0 in (a["w0"], 40.0, -40.0):
        fm.w0 = w0
        got = check_scores(fm, ds, a["y"], a["c"])
        check_scores(fm, dss, a["y"], a["c"])
        assert fm.computeRMSE(ds) == fm.computeRMSE(plain) and fm.computeLogLoss(ds) == fm.computeLogLoss(plain)
    fm.w0 = a["w0"]
    lone = fm.weightedScores(ds)
    seen = [None, None]

    def score(i):
        seen[i] = [fm.weightedScores(ds) for _ in range(5)]
    fm.handle                                                      # (the upload happens once, before the threads share the model)
    threads = [threading.Thread(target=score, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert all(s == lone for s in seen[0] + seen[1])
    # a non-finite prediction: counted whatever the row's weight; it spoils the ratios only through rows that count
    f = int(a["col"][a["row_ptr"][10]])
    rows_f = np.array([f in a["col"][a["row_ptr"][r]:a["row_ptr"][r + 1]] for r in range(1500)])
    w = a["w"].copy()
    w[f] = np.inf
    fm.w = w
    c0 = a["c"].copy()
    c0[rows_f] = 0.0
    ds0, _ = make(fmhip, a, weights=c0)
    got = fm.weightedScores(ds0)
    assert got["nonfinite"] == int(rows_f.sum()) > 0 and np.isfinite(got["rmse"]) and np.isfinite(got["logloss"])
    want = wref.weighted_scores(np.where(rows_f, 0.0, fm.predict(ds0)), a["y"], c0)
    assert got["rmse"] == pytest.approx(want["rmse"], rel=1e-5) and got["logloss"] == pytest.approx(want["logloss"], rel=1e-5)
    assert not np.isfinite(fm.weightedScores(ds)["rmse"])
    fm.w = a["w"]
    # sum c == 0
    dsz, _ = make(fmhip, a, weights=np.zeros(1500))
    z = fm.weightedScores(dsz)
    assert z["sum_w"] == 0.0 and z["rows"] == 1500 and all(np.isnan(z[key]) for key in ("rmse", "mae", "logloss"))
    for d in (ds, dss, plain, ds0, dsz):
        d.unpersist()
    fm.close()


def test_weighted_scores_of_a_lazily_decayed_model(fmhip):
    """A wide model after rows-only steps with decay (the tables hold U with V = sv U, sv != 1): the scores are those of the
    parameters the model reads back."""
    a = problem(811, 800, 20000, 64, 2, 10, "logistic")
    ds, fm = make(fmhip, a, batch_rows=100)
    sgd = fmhip.HipSGD(eta=0.1, reg0=1e-3, regw=1e-3, regv=2e-3, loss="logistic")
    for b in range(4):
        sgd.step(fm, ds, b)
    got = fm.weightedScores(ds)                                    # scored with the scale pending
    check_scores(fm, ds, a["y"], a["c"])
    fm2 = fmhip.FMModel(a["n1"] - 1, a["k"])
    fm2.w0, fm2.w, fm2.v = fm.w0, fm.w, fm.v                       # the same parameters at scale 1
    folded = fm2.weightedScores(ds)
    for key in ("rmse", "mae", "logloss"):
        assert got[key] == pytest.approx(folded[key], rel=1e-5), key
    assert np.abs(fm.v - a["v"]).max() > 1e-4
    ds.unpersist()
    fm.close()
    fm2.close()


# ---- 9. include/sparkfm.hpp ----------------------------------------------------------------------------------------------------

def test_cpp_weighted_step_and_scores_match_the_python_mirror(fmhip, tmp_path):
    """tests/cpp_weights.cpp builds a small weighted dataset and a model from integer formulas, runs one HipSGD epoch and
    FMModel::weightedScores through include/sparkfm.hpp and prints every number as a hex float; the Python mirror over the same
    formulas gives the same bits."""
    from sparkfm_amd import _build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_weights")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_weights.cpp"), "-L" + _build.LIBDIR, "-lfmhip",
                           "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    out = {}
    for line in r.stdout.decode().split("\n"):
        if line.strip():
            key, *vals = line.split()
            out[key] = [float.fromhex(x) for x in vals]
    n_rows, n1, k = 1000, 301, 8
    rows, weights = [], []
    for r_ in range(n_rows):
        idx, val, y = [], [], 0.5
        for j in range(3 + r_ % 6):
            i = (r_ * 13 + j * 101 + (r_ * j) % 7) % n1
            if i in idx:
                continue
            x = 0.5 + ((r_ + j) % 4) / 8.0
            idx.append(i)
            val.append(x)
            y += x * ((i % 5) - 2) * 0.2
        rows.append((y, (idx, val)))
        weights.append([0.0, 0.25, 1.0, 3.5, 1.0][r_ % 5])
    ds = fmhip.DataSet.from_rows(rows, weights=weights, batch_rows=250).cache()
    fm = fmhip.FMModel(n1 - 1, k)
    fm.w0 = 0.1
    fm.w = [0.02 * ((i % 7) - 3) for i in range(n1)]
    fm.v = np.array([[0.01 * ((f * 7 + i * 3) % 11 - 5) for i in range(n1)] for f in range(k)])
    before = fm.weightedScores(ds)
    fmhip.HipSGD(eta=0.05, reg0=0.0, regw=1e-4, regv=1e-4).learn(fm, ds)
    after = fm.weightedScores(ds)
    assert out["before"] == [before["sum_w"], before["rmse"], before["mae"], before["logloss"]]
    assert out["after"] == [after["sum_w"], after["rmse"], after["mae"], after["logloss"]]
    assert out["w0"] == [fm.w0] and out["w"] == fm.w.tolist() and out["v"] == fm.v.reshape(-1, order="F").tolist()
    assert after["rmse"] < before["rmse"] and before["sum_w"] == sum(weights)
    ds.unpersist()
    fm.close()
