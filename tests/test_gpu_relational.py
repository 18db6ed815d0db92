"""Relational data on the device (include/fmhip_relational.h): the relational step, epochs and scores against the fp64 twin by block
caches (relational_ref.py, pinned to the flat step by test_host_relational.py) and against the flat path on expand(); the segmented
sum's edges; rows nobody references; the refusals; the fit loop; include/sparkfm.hpp.

Tolerances are the project's: check_step of test_gpu_weights.py (TOL_G per feature) and of test_gpu_adagrad.py for one step, TOL_Y of
test_gpu_parity.py for predictions, rel 1e-5 for the scores and the step's statistics, rel-L2 1e-5 for trajectories."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import relational_ref as rref
import train_ref as ref
from test_gpu_adagrad import EPS, check_step as check_adagrad_step, get_state
from test_gpu_parity import TOL_Y, term_scale
from test_gpu_weights import check_step
from train_ref import rel, same

pytestmark = pytest.mark.gpu

REGS = (1e-3, 2e-3, 3e-3)
ETA = 0.05


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def L():
    from sparkfm_amd import _ffi
    return _ffi.load()


def params(fm):
    return fm.w0, fm.w.copy(), fm.v.copy()


def close(rd, fm):
    rd.unpersist()
    for part in rd._parts():
        part.unpersist()
    fm.close()


def one_step(fmhip, p, loss, regs=REGS, batch_rows=0, batch=0, hot_block=None, **kw):
    """One relational step of `batch` on the device and by the twin -> (fm, rd, s0, s1, stats, e).  hot_block: relational_ref.build's."""
    rd, fm = rref.build(fmhip, p, batch_rows, hot_block)
    n = len(p["y"])
    br = batch_rows if 0 < batch_rows <= n else n
    r0, r1 = batch * br, min(n, (batch + 1) * br)
    init = kw.get("adagrad_init", 0.0)
    s0 = ref.State(p["w0"], p["w"], p["v"], init)
    rule = ref.Rule(loss, False, EPS if kw.get("optimizer") == "adagrad" else None)
    e = rref.residuals(s0, p, r0, r1, loss)
    s1 = rref.step(s0.copy(), p, r0, r1, ETA, *regs, rule)
    st = fmhip.HipSGD(eta=ETA, reg0=regs[0], regw=regs[1], regv=regs[2], loss=loss, **kw).step(fm, rd, batch)
    return fm, rd, s0, s1, st, e


def check_stats(st, e):
    """rows, sse and sum_e to rel 1e-5.  sum_e is a sum of residuals of both signs that can cancel to a small fraction of its terms,
    so it carries the absolute floor 1e-4 beside the relative bound — the form and the constant of test_gpu_weights.py's check of
    the same statistic (fp32 rounding of a few hundred terms of size <= a few: 400 * 3 * 6e-8 = 7e-5), not a wider relative bound."""
    assert st["rows"] == len(e) and st["nonfinite"] == 0 and st["steps"] == 1
    assert st["sse"] == pytest.approx((e * e).sum(), rel=1e-5) and st["sum_e"] == pytest.approx(e.sum(), rel=1e-5, abs=1e-4)


# ---- 1. one step against the twin -----------------------------------------------------------------------------------------

# k -> (Kp, packed w slot?): 8 / 32 (Kp 32), 48 / 64 (Kp 64), 100 / 128 (Kp 128), 200 / 256 (Kp 256)
KS = [8, 32, 48, 64, 100, 128, 200, 256]


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k", KS)
def test_one_step_vs_twin(fmhip, k, loss):
    """fmhip_relational_sgd_step on the base problem (a block row referenced 150 times, block rows nobody references, an empty block
    row, a plain part): V, w, w0 and the step's statistics."""
    p = rref.base_problem(200 + k, k, loss)
    fm, rd, s0, s1, st, e = one_step(fmhip, p, loss)
    check_step(fm, s0, s1)
    check_stats(st, e)
    assert rd.info() == dict(n_rows=400, dimension=rd.dimension, batch_rows=400, n_batches=1, n_relations=2)
    close(rd, fm)


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k", [32, 100])
def test_one_adagrad_step_vs_twin(fmhip, k, loss):
    p = rref.base_problem(300 + k, k, loss)
    fm, rd, s0, s1, st, e = one_step(fmhip, p, loss, optimizer="adagrad", adagrad_init=0.1)
    check_adagrad_step(fm, s0, s1, 0.1, ETA)
    check_stats(st, e)
    close(rd, fm)


# ---- 2. predictions and scores ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [8, 64, 100, 256])
def test_predictions_and_scores(fmhip, k):
    """fm.predict(rel) against fm.predict(rel.expand()) (2 x TOL_Y: two fp32 paths) and against the oracle (TOL_Y), computeRMSE and
    computeLogLoss to rel 1e-5 — on the training object, before and after three training steps."""
    import oracle
    p = rref.base_problem(400 + k, k, "logistic", n_rows=900)
    rd, fm = rref.build(fmhip, p, batch_rows=300)
    fl = rd.expand().cache()
    a = rref.flat(p)
    sgd = fmhip.HipSGD(eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2], loss="logistic")
    for trained in (False, True):
        if trained:
            for b in (0, 1, 2):
                sgd.step(fm, rd, b)
        w0, w, v = params(fm)
        oy = oracle.predict(w0, w, v, a["row_ptr"], a["col"], a["val"])
        sc = term_scale(dict(a, w0=w0, w=w, v=v))
        yr, yf = fm.predict(rd), fm.predict(fl)
        assert (np.abs(yr - oy) <= TOL_Y * sc).all(), float((np.abs(yr - oy) / sc).max())
        assert (np.abs(yr - yf) <= 2 * TOL_Y * sc).all(), float((np.abs(yr - yf) / sc).max())
        assert fm.computeRMSE(rd) == pytest.approx(np.sqrt(((oy - p["y"]) ** 2).mean()), rel=1e-5)
        t = p["y"] > 0
        assert fm.computeLogLoss(rd) == pytest.approx((ref.softplus(oy) - t * oy).mean(), rel=1e-5)
        acc = float((((p["y"] >= 0) & (oy >= 0)) | ((p["y"] < 0) & (oy < 0))).mean())
        assert abs(fm.computeAccuracy(rd) - acc) <= (np.abs(oy) <= TOL_Y * sc).mean()       # (rows whose sign the tolerance leaves open)
        assert np.array_equal(fm.predict(rd), yr)                    # scoring is a pure function of the model
    assert np.abs(fm.v - p["v"]).max() > 1e-4                        # the second round scored a trained model
    fl.unpersist()
    close(rd, fm)


# ---- 3. epochs ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,loss", [(32, "squared"), (130, "logistic")])
def test_epochs_vs_twin(fmhip, k, loss):
    """Two shuffled epochs, 900 rows in batches of 200 (the last one short): rel-L2 1e-5 on v and w against the twin; the same run
    on expand() through the flat path is within the same bound of the twin; both moved."""
    p = rref.base_problem(500 + k, k, loss, n_rows=900)
    rd, fm = rref.build(fmhip, p, batch_rows=200)
    fl = rd.expand().cache()
    fm2 = fmhip.FMModel(p["n1"] - 1, k)
    fm2.w0, fm2.w, fm2.v = p["w0"], p["w"], p["v"]
    assert rd.n_batches == 5 == fl.n_batches
    orders = []
    for model, data in ((fm, rd), (fm2, fl)):
        sgd = fmhip.HipSGD(eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2], shuffle_seed=3, loss=loss)
        orders = []
        for _ in range(2):
            orders.append(sgd.batch_order(5).tolist())
            sgd.learn(model, data)
        assert sgd.last_stats["rows"] == 900 and sgd.last_stats["steps"] == 5
    s = rref.epochs(ref.State(p["w0"], p["w"], p["v"]), p, 200, orders, ETA, *REGS, ref.Rule(loss, False, None))
    for model in (fm, fm2):
        assert rel(model.v, s.v) <= 1e-5 and rel(model.w, s.w) <= 1e-5, (rel(model.v, s.v), rel(model.w, s.w))
        assert model.w0 == pytest.approx(s.w0, rel=1e-5, abs=1e-6)
        assert np.abs(model.w - p["w"]).max() > 1e-4                # it moved
    fl.unpersist()
    fm2.close()
    close(rd, fm)


# ---- 4. the segmented sum's edges ----------------------------------------------------------------------------------------

def edge_problem(case, k, loss):
    """-> (problem, batch_rows, batch).  The cut is FMHIP_RELATIONAL_SUM_CUT rows: a longer list is summed in chunks."""
    from sparkfm_amd import _ffi
    cut = _ffi.RELATIONAL_SUM_CUT
    rng = np.random.default_rng(77)
    users = rref.random_block(rng, 20, 1, 5, 0, 100)
    items = rref.random_block(rng, 12, 1, 6, 100, 220)
    if case == "lengths":
        # item rows 1..4 referenced 1, cut - 1, cut, cut + 1 times, row 0 never, the rest by the other rows
        lens = [1, cut - 1, cut, cut + 1]
        mi = np.concatenate([np.full(n, j + 1) for j, n in enumerate(lens)] + [rng.integers(5, 12, 900 - sum(lens))])
        rng.shuffle(mi)
        p = rref.make_problem(1, 900, k, [users, items], [rng.integers(0, 20, 900), mi], rref.random_block(rng, 900, 0, 3, 220, 300), 300, loss)
        return p, 0, 0
    if case == "every_row":       # one block row referenced by every row of the batch: three chunks
        p = rref.make_problem(2, 3 * cut - 7, k, [users, items], [rng.integers(0, 20, 3 * cut - 7), np.full(3 * cut - 7, 6)], None, 300, loss)
        return p, 0, 0
    if case == "one_block_row":   # J_b = 1
        one = rref.random_block(rng, 1, 4, 4, 0, 100)
        p = rref.make_problem(3, 300, k, [one, items], [np.zeros(300, np.int64), rng.integers(0, 12, 300)], rref.random_block(rng, 300, 0, 3, 220, 300), 300, loss)
        return p, 0, 0
    if case == "short_batch":     # 450 rows in batches of 200: the step on the last, short batch
        p = rref.make_problem(4, 450, k, [users, items], [rng.integers(0, 20, 450), rng.integers(0, 12, 450)], rref.random_block(rng, 450, 0, 3, 220, 300), 300, loss)
        return p, 200, 2
    if case == "one_relation":    # m = 1 and no plain part
        p = rref.make_problem(5, 300, k, [items], [rng.integers(0, 12, 300)], None, 300, loss)
        return p, 0, 0
    assert case == "three_relations"
    third = rref.random_block(rng, 7, 0, 4, 220, 260)
    p = rref.make_problem(6, 300, k, [users, items, third], [rng.integers(0, 20, 300), rng.integers(0, 12, 300), rng.integers(0, 7, 300)],
                          rref.random_block(rng, 300, 0, 3, 260, 300), 300, loss)
    return p, 0, 0


@pytest.mark.parametrize("k,loss", [(8, "squared"), (64, "logistic")])
@pytest.mark.parametrize("case", ["lengths", "every_row", "one_block_row", "short_batch", "one_relation", "three_relations"])
def test_segmented_sum_edges(fmhip, case, k, loss):
    """One step against the twin, and two runs that are bit-identical (packed rows at k = 8, the residual embedded in the row at
    k = 64)."""
    p, batch_rows, batch = edge_problem(case, k, loss)
    outs = []
    for _ in range(2):
        fm, rd, s0, s1, st, e = one_step(fmhip, p, loss, batch_rows=batch_rows, batch=batch)
        check_step(fm, s0, s1)
        check_stats(st, e)
        outs.append(params(fm) + (st["sse"], st["sum_e"]))
        close(rd, fm)
    assert same(outs[0], outs[1])


# ---- 4b. parts with a dense hot block ---------------------------------------------------------------------------------------

HOT_BATCH = 100


def assert_hot_parts(rd, p):
    """base_problem(hot=True) built with hot_block=4 and in batches: the user block and the plain part both report the hot block the
    library's rule gives them (relational_ref.hot_layouts), with the dense features in it."""
    want_u, want_p = rref.hot_layouts(p, HOT_BATCH)
    got_u, got_p = rd.relations[0].block.layout(), rd.plain.layout()
    for got, want, dense in ((got_u, want_u, rref.DEMO), (got_p, want_p, rref.PLAIN_HOT)):
        assert got["hot_pages"] == want["hot_pages"] >= 1 and sorted(got["hot_ids"]) == want["hot_ids"] and sorted(got["hot_ids_all"]) == want["hot_ids_all"]
        assert set(dense) <= set(got["hot_ids_all"]) and len(set(dense) & set(got["hot_ids"])) >= 2
        assert got["nnz_sparse_backward"] == want["nnz_sparse_backward"]
    assert rref.DEMO_UNREFERENCED in got_u["hot_ids"] and rd.plain.n_batches == 4
    assert rd.relations[1].block.layout()["hot_pages"] == 0          # the item block: single-batch, not asked for by name


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k", [8, 32, 100])
@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
def test_hot_block_parts_one_step_vs_twin_and_flat(fmhip, optimizer, k, loss):
    """base_problem(hot=True): six dense "demographic" features in the user block (built with hot_block=4: the block product reads
    the block's gathered Pb / eb), three in the plain part (four batches of 100 rows).  One step of every batch against the
    relational twin and the device's own flat step on expand() against the same twin, at check_step's bounds (test_gpu_weights.py /
    test_gpu_adagrad.py); the statistics; two runs bit-identical."""
    p = rref.base_problem(700 + k, k, loss, hot=True)
    kw = dict(optimizer="adagrad", adagrad_init=0.1) if optimizer == "adagrad" else {}
    for b in range(4):
        outs = []
        for _ in range(2):
            fm, rd, s0, s1, st, e = one_step(fmhip, p, loss, batch_rows=HOT_BATCH, batch=b, hot_block=4, **kw)
            outs.append(params(fm) + (get_state(fm) if kw else ()) + (st["sse"], st["sum_e"]))
            if len(outs) == 2:
                break
            assert_hot_parts(rd, p)
            check_stats(st, e)
            fl = rd.expand().cache()
            fm2 = fmhip.FMModel(p["n1"] - 1, k)
            fm2.w0, fm2.w, fm2.v = p["w0"], p["w"], p["v"]
            fmhip.HipSGD(eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2], loss=loss, **kw).step(fm2, fl, b)
            for model in (fm, fm2):
                if kw:
                    check_adagrad_step(model, s0, s1, 0.1, ETA)
                else:
                    check_step(model, s0, s1)
            fl.unpersist()
            fm2.close()
            close(rd, fm)
        close(rd, fm)
        assert same(outs[0], outs[1]), b


@pytest.mark.parametrize("k", [8, 32, 100])
@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
def test_unreferenced_block_rows_leave_a_hot_feature_untouched(fmhip, optimizer, k):
    """Feature 99 sits in page 0 of the user block's hot block and only in block rows no data row references: the block product
    reads exact zeros from Pb / eb there, so its gradient is exactly zero as the twin's is — without decay its v row, its w and (AdaGrad)
    its accumulators keep every bit, while the other dense features move."""
    p = rref.base_problem(700 + k, k, "squared", hot=True)
    f = rref.DEMO_UNREFERENCED
    assert not np.isin(np.flatnonzero(rref.dense(p["blocks"][0]["row_ptr"], p["blocks"][0]["col"], p["blocks"][0]["val"], p["n1"])[:, f]), p["maps"][0]).any()
    kw = dict(optimizer="adagrad", adagrad_init=0.1) if optimizer == "adagrad" else {}
    for b in range(4):
        fm, rd, s0, s1, st, e = one_step(fmhip, p, "squared", regs=(0.0, 0.0, 0.0), batch_rows=HOT_BATCH, batch=b, hot_block=4, **kw)
        assert_hot_parts(rd, p)
        assert s1.w[f] == s0.w[f] and np.array_equal(s1.v[:, f], s0.v[:, f])             # the twin: an exactly zero gradient
        assert fm.w[f] == np.float32(p["w"][f]) and np.array_equal(fm.v[:, f], p["v"][:, f].astype(np.float32))
        moved = [g for g in rref.DEMO if g != f]
        assert (fm.v[:, moved] != p["v"][:, moved].astype(np.float32)).any(axis=0).all()
        if kw:
            n0, nw, nv = get_state(fm)
            assert nw[f] == np.float32(0.1) and (nv[:, f] == np.float32(0.1)).all() and (nv[:, moved] > np.float32(0.1)).any(axis=0).all()
        close(rd, fm)


def test_two_models_take_turns_on_one_handle(fmhip):
    """The workspace is the handle's and a step returns before it has run: two models (each with a stream of its own) stepping
    alternately on ONE RelationalData, no statistics read and no synchronise in between, end with the bits each of them reaches
    alone on a handle of its own."""
    p = rref.base_problem(650, 32, n_rows=900)
    q = dict(p, w0=-p["w0"], w=p["w"][::-1].copy(), v=p["v"][:, ::-1].copy())
    sgd = fmhip.HipSGD(eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2])
    alone = []
    for prob in (p, q):
        rd, fm = rref.build(fmhip, prob, batch_rows=300)
        for _ in range(3):
            for b in (0, 1, 2):
                sgd.step(fm, rd, b, want_stats=False)
        alone.append(params(fm))
        close(rd, fm)
    rd, fm1 = rref.build(fmhip, p, batch_rows=300)
    fm2 = fmhip.FMModel(p["n1"] - 1, 32)
    fm2.w0, fm2.w, fm2.v = q["w0"], q["w"], q["v"]
    for _ in range(3):
        for b in (0, 1, 2):
            sgd.step(fm1, rd, b, want_stats=False)
            sgd.step(fm2, rd, b, want_stats=False)
    assert same(params(fm1), alone[0]) and same(params(fm2), alone[1])
    assert not same(alone[0], alone[1])
    fm2.close()
    close(rd, fm1)


# ---- 5. rows nobody references ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
@pytest.mark.parametrize("k", [32, 100])
def test_unreferenced_block_rows_have_a_zero_gradient(fmhip, k, optimizer):
    """The features that occur only in block rows nobody references: with reg = 0 their parameters keep their bits, and under AdaGrad
    their accumulators stay at the initial value — their gradient is exactly zero."""
    p = rref.base_problem(600 + k, k)
    used = set()
    for b, m in zip(p["blocks"], p["maps"]):
        for j in np.unique(m):
            used.update(b["col"][b["row_ptr"][j]:b["row_ptr"][j + 1]].tolist())
    every = set(np.concatenate([b["col"] for b in p["blocks"]]).tolist())
    only = np.array(sorted(every - used))
    assert len(only) >= 5
    fm, rd, s0, s1, st, e = one_step(fmhip, p, "squared", regs=(0.0, 0.0, 0.0), optimizer=optimizer, adagrad_init=0.1)
    assert np.array_equal(fm.v[:, only], p["v"][:, only].astype(np.float32)) and np.array_equal(fm.w[only], p["w"][only].astype(np.float32))
    if optimizer == "adagrad":
        _, nw, nv = get_state(fm)
        assert (nv[:, only] == np.float32(0.1)).all() and (nw[only] == np.float32(0.1)).all()
        touched = np.array(sorted(used))
        assert (nv[:, touched] > np.float32(0.1)).any(axis=0).mean() > 0.9
    assert np.abs(fm.v - p["v"]).max() > 1e-4               # the others moved
    close(rd, fm)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------

def test_a_model_set_to_pairs_is_refused_unchanged(fmhip):
    from sparkfm_amd import _ffi
    p = rref.base_problem(700, 8)
    rd, fm = rref.build(fmhip, p)
    _ = fm.handle
    fm._host_fresh = False
    before = params(fm)                                      # as the device holds them (fp32)
    sgd = fmhip.HipSGD(eta=ETA, loss="logistic", pairs=True)
    for call in (lambda: sgd.step(fm, rd, 0), lambda: sgd.learn(fm, rd)):
        with pytest.raises(_ffi.FmhipError, match="pairs") as ei:
            call()
        assert ei.value.code == -5
    fm._host_fresh = False
    assert same(params(fm), before)
    st = fmhip.HipSGD(eta=ETA).step(fm, rd, 0)               # the same objects train once the pairing is off
    assert st["rows"] == 400 and np.abs(fm.v - before[2]).max() > 1e-5
    close(rd, fm)


def test_create_refuses_and_names_the_item(fmhip):
    """The C call's own refusals (they need block handles): a weighted block and a scoring block (-5), a block with several batches,
    a mapping entry out of range, a shared feature, a plain part of another shape (-1) — each message names the item."""
    from sparkfm_amd import DataSet, _ffi
    rng = np.random.default_rng(5)
    ub, ib = rref.random_block(rng, 6, 1, 3, 0, 20), rref.random_block(rng, 9, 1, 3, 20, 50)
    n = 40
    y = rng.normal(0, 1, n)
    mu, mi = rng.integers(0, 6, n).astype(np.int32), rng.integers(0, 9, n).astype(np.int32)
    mk = lambda b, **kw: DataSet(b["row_ptr"], b["col"], b["val"], np.zeros(len(b["row_ptr"]) - 1), **kw).cache()      # noqa: E731
    users, items = mk(ub), mk(ib)

    def create(blocks, maps, plain=None, batch_rows=0):
        h = C.c_void_p(7)
        hb = (C.c_void_p * len(blocks))(*[b.handle for b in blocks])
        hm = (C.c_void_p * len(maps))(*[_ffi.ptr(m) for m in maps])
        rc = L().fmhip_relational_create(0, n, _ffi.ptr(y), len(blocks), hb, hm, None if plain is None else plain.handle, batch_rows, C.byref(h))
        assert (rc == 0) == (h.value is not None)
        if rc == 0:
            L().fmhip_relational_destroy(h)
        return rc, L().fmhip_last_error().decode()

    assert create([users, items], [mu, mi])[0] == 0
    weighted, scoring, batched = mk(ib, weights=np.ones(9)), mk(ib, scoring=True), mk(ib, batch_rows=4)
    rc, msg = create([users, weighted], [mu, mi])
    assert rc == -5 and "relation 1" in msg and "weight" in msg, msg
    rc, msg = create([users, scoring], [mu, mi])
    assert rc == -5 and "relation 1" in msg and "scoring" in msg, msg
    rc, msg = create([users, batched], [mu, mi])
    assert rc == -1 and "relation 1" in msg and "3 batches" in msg, msg
    bad = mi.copy()
    bad[17], bad[30] = 9, -1
    rc, msg = create([users, items], [mu, bad])
    assert rc == -1 and "relation 1" in msg and "mapping[17] = 9" in msg and "[0, 9)" in msg, msg
    shared = dict(ib, col=ib["col"].copy())
    shared["col"][shared["col"] == shared["col"].max()] = ub["col"][0]       # the items' last feature becomes one of the users'
    rc, msg = create([users, mk(shared)], [mu, mi])
    assert rc == -1 and "feature %d occurs in relation 0 and in relation 1" % ub["col"][0] in msg, msg
    pb = rref.random_block(rng, n, 0, 2, 50, 60)
    plain = DataSet(pb["row_ptr"], pb["col"], pb["val"], y, batch_rows=16).cache()
    assert create([users, items], [mu, mi], plain, 16)[0] == 0
    rc, msg = create([users, items], [mu, mi], plain, 10)
    assert rc == -1 and "plain part is batched by 16" in msg, msg
    short = rref.random_block(rng, n - 1, 0, 2, 50, 60)
    rc, msg = create([users, items], [mu, mi], DataSet(short["row_ptr"], short["col"], short["val"], y[:-1]).cache())
    assert rc == -1 and "plain part has 39 rows" in msg, msg
    pshared = dict(pb, col=np.where(pb["col"] == pb["col"].min(), ib["col"][0], pb["col"]).astype(np.int32))
    rc, msg = create([users, items], [mu, mi], DataSet(pshared["row_ptr"], pshared["col"], pshared["val"], y).cache())
    assert rc == -1 and "feature %d occurs in relation 1 and in the plain part" % ib["col"][0] in msg, msg
    # through the Python classes: the weighted block reaches the library and comes back as FmhipError
    with pytest.raises(_ffi.FmhipError, match="weight") as ei:
        fmhip.RelationalData(y, [fmhip.Relation(users, mu), fmhip.Relation(weighted, mi)]).cache()
    assert ei.value.code == -5
    # a model that is too narrow
    fm = fmhip.FMModel(10, 4)
    rd = fmhip.RelationalData(y, [fmhip.Relation(users, mu), fmhip.Relation(items, mi)])
    with pytest.raises(_ffi.FmhipError, match="num_attribute") as ei:
        fmhip.HipSGD().step(fm, rd, 0)
    assert ei.value.code == -4
    with pytest.raises(_ffi.FmhipError, match="batch 1 out of range"):
        fmhip.HipSGD().step(fmhip.FMModel(60, 4), rd, 1)


# ---- 7. the fit loop -------------------------------------------------------------------------------------------------------

def test_fit_loop_with_relations(fmhip):
    """FM(ds, 8).withRelation([users, items]).learnWith(HipSGD.run(...)) lowers the RMSE over 3 iterations and equals the explicit
    RelationalData run bit for bit."""
    p = rref.base_problem(800, 8, n_rows=900)
    truth = ref.State(0.3, np.random.default_rng(1).normal(0, 0.5, 300), np.random.default_rng(2).normal(0, 0.3, (8, 300)))
    y = rref.predict(truth, p)
    users, items = [fmhip.Relation((b["row_ptr"], b["col"], b["val"]), m) for b, m in zip(p["blocks"], p["maps"])]
    ds = fmhip.DataSet(p["plain"]["row_ptr"], p["plain"]["col"], p["plain"]["val"], y, batch_rows=300, name="ratings")
    kw = dict(eta=0.1, reg0=0.0, regw=1e-4, regv=1e-4)
    fit = fmhip.FM(ds, 8, maxIteration=3, seed=4).withRelation([users, items])
    fm = fit.learnWith(fmhip.HipSGD.run(**kw))
    h = fit.rmse_history
    assert len(h) == 3 and h[0] > h[1] > h[2] > 0
    rd = fmhip.RelationalData(y, [users, items], plain=ds, batch_rows=300)
    fm2 = fmhip.FMModel(rd.dimension, 8, seed=4)
    sgd, h2 = fmhip.HipSGD.run(**kw), []
    for _ in range(3):
        h2.append(fm2.computeRMSE(rd))
        sgd.learn(fm2, rd)
    assert h2 == h and same(params(fm), params(fm2))
    assert fm2.computeRMSE(rd) < h[2]
    fm2.close()
    close(rd, fm)


# ---- 8. include/sparkfm.hpp ------------------------------------------------------------------------------------------------

def cpp_problem():
    """The integer formulas of tests/cpp_relational.cpp."""
    n, nu, ni, k = 600, 23, 41, 8
    def block(rows, base, span, mul):
        rp, col, val = [0], [], []
        for j in range(rows):
            seen = []
            for t in range(1 + j % 4):
                i = base + (j * mul + t * 17 + (j * t) % 5) % span
                if i not in seen:
                    seen.append(i)
                    col.append(i)
                    val.append(0.5 + ((j + t) % 4) / 8.0)
            rp.append(len(col))
        return dict(row_ptr=np.asarray(rp, np.int64), col=np.asarray(col, np.int32), val=np.asarray(val))
    users, items = block(nu, 0, 60, 7), block(ni, 60, 90, 11)
    mu = np.array([(r * 5 + r // 7) % nu for r in range(n)], np.int32)
    mi = np.array([3 if r % 3 == 0 else (r * 11 + r // 5) % ni for r in range(n)], np.int32)
    prp, pcol, pval = [0], [], []
    for r in range(n):
        for t in range(r % 3):
            pcol.append(150 + (r * 3 + t * 7) % 30 if t == 0 else 180 + (r + t) % 20)
            pval.append(1.0 if t == 0 else 0.25)
        prp.append(len(pcol))
    y = np.array([0.5 + 0.1 * ((r * 7) % 11 - 5) for r in range(n)])
    n1 = 200
    w = np.array([0.02 * ((i % 7) - 3) for i in range(n1)])
    v = np.array([[0.01 * ((f * 7 + i * 3) % 11 - 5) for i in range(n1)] for f in range(k)])
    plain = dict(row_ptr=np.asarray(prp, np.int64), col=np.asarray(pcol, np.int32), val=np.asarray(pval))
    return dict(k=k, n1=n1, w0=0.1, w=w, v=v, y=y, blocks=[users, items], maps=[mu, mi], plain=plain)


def test_cpp_relational_matches_python(fmhip, tmp_path):
    """tests/cpp_relational.cpp (include/sparkfm.hpp's Relation / RelationalData) against the Python mirror over the same integer
    formulas: RMSE before and after one epoch in batches of 250, and every parameter, hex floats equal."""
    from sparkfm_amd import _build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_relational")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_relational.cpp"), "-L" + _build.LIBDIR, "-lfmhip",
                           "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = {ln.split()[0]: [float.fromhex(t) for t in ln.split()[1:]] for ln in out.stdout.decode().splitlines()}
    p = cpp_problem()
    rd, fm = rref.build(fmhip, p, batch_rows=250)
    before = fm.computeRMSE(rd)
    fmhip.HipSGD.run(eta=0.05, reg0=0.0, regw=1e-4, regv=1e-4).learn(fm, rd)
    assert got["before"] == [before] and got["after"] == [fm.computeRMSE(rd)] and got["after"][0] < before
    assert got["w0"] == [fm.w0] and got["w"] == fm.w.tolist() and got["v"] == fm.v.reshape(-1, order="F").tolist()
    assert got["predict3"] == fm.predict(rd)[:3].tolist()
    close(rd, fm)
