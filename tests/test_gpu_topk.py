"""GPU checks of top-K recommendation (include/fmhip_topk.h: fmhip_topk, fmhip_pair_scores; FMModel.recommend / pairScores).

Oracle: the fp64 oracle's predict and fp64 numpy q through the pair identity
    score(c, d) = predict(c) + predict(d) - w0 + sum_f q_f(c) q_f(d)
(pinned on the CPU in tests/test_host_topk.py), so no test needs B x M joined rows.  Score tolerance: the project's TOL_Y = 1e-5
times (1 + sum |terms|) of the joined row — the terms of c, the terms of d, sum_f |q_f(c) q_f(d)| (tests/topk_ref.py)."""
import os
import subprocess
import threading
import time

import numpy as np
import pytest

import oracle
from topk_ref import check_topk, field_rows, joined, pair_ref, params, row_stats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def dataset(fmhip, r, scoring=True, batch_rows=0):
    return fmhip.DataSet(r["row_ptr"], r["col"], r["val"], np.zeros(len(r["row_ptr"]) - 1), scoring=scoring, batch_rows=batch_rows).cache()


def model(fmhip, n1, k, w0, w, v):
    fm = fmhip.FMModel(n1 - 1, k)
    fm.w0, fm.w, fm.v = w0, w, v
    return fm


def problem(seed, B, M, n1, k, empty_c=(), empty_d=(), scale=0.1):
    """contexts over ids [0, n1/2), candidates over [n1/2, n1): three fields a side"""
    h = n1 // 2
    w0, w, v = params(seed, n1, k, scale)
    ctx = field_rows(seed + 100, B, [(0, h // 2), (h // 2, h - 8), (h - 8, h)], empty=empty_c, half=False)
    cand = field_rows(seed + 200, M, [(h, h + h // 2), (h + h // 2, n1 - 8), (n1 - 8, n1)], empty=empty_d, half=False)
    return w0, w, v, ctx, cand


# ---- 1. fmhip_pair_scores vs the oracle -----------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 8, 31, 32, 33, 64, 100, 128, 200, 256])
def test_pair_scores_match_the_oracle(fmhip, k):
    """Every pair of 37 x 1,003 rows (neither a multiple of 16), all four padded widths, packed (k < Kp: the packed slot is
    in the first float4 for k = 1, in the last for k = 31 / 200) and unpacked (k = 32, 64, 128, 256) rows, empty rows on
    both sides, and a candidate that shares a feature with the contexts (the oracle is the identity's right-hand side)."""
    n1 = 400
    w0, w, v, ctx, cand = problem(k, 37, 1003, n1, k, empty_c=(0, 17, 36), empty_d=(0, 500, 1002))
    cand["col"][cand["row_ptr"][5]] = 3                     # candidate 5 holds a context-side id
    ctx["col"][ctx["row_ptr"][2]] = 3                       # ... which context 2 holds too
    S, tol = pair_ref(w0, w, v, ctx, cand)
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    got = fm.pairScores(dc, dd)
    assert got.shape == (37, 1003)
    print("k=%d max |d|/tol = %.3f" % (k, float((np.abs(got - S) / tol).max())))
    assert (np.abs(got - S) <= tol).all(), float((np.abs(got - S) / tol).max())
    assert got[0, 0] == np.float32(w0)                      # empty x empty
    # a sub-range of the contexts, from a TRAINING dataset cut into small batches (its forward may sum a row in another order:
    # the dense hot block)
    dt = dataset(fmhip, ctx, scoring=False, batch_rows=10)
    sub = fm.pairScores(dt, dd, 7, 29)
    assert sub.shape == (22, 1003) and (np.abs(sub - S[7:29]) <= tol[7:29]).all()
    np.testing.assert_array_equal(fm.pairScores(dc, dd, 7, 29), got[7:29])
    assert fm.pairScores(dc, dd, 5, 5).shape == (0, 1003)
    for d in (dc, dd, dt):
        d.unpersist()
    fm.close()


@pytest.mark.parametrize("k", [16, 32])
def test_pair_scores_of_a_lazily_decayed_model(fmhip, k):
    """A wide model after rows-only updates with weight decay holds V = sv * U (sv != 1): the forward folds the scales into q
    and yhat, so the scores are those of the parameters the model reports."""
    from helpers import random_problem
    a = random_problem(5, 300, 5000, k, 2, 8)
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=100).cache()
    fm = model(fmhip, a["n1"], k, a["w0"], a["w"], a["v"])
    sgd = fmhip.HipSGD(eta=0.5, reg0=0.0, regw=0.2, regv=0.2)
    for _ in range(2):
        sgd.learn(fm, ds)
    ctx = field_rows(1, 21, [(0, 1000), (1000, 2500)], empty=(3,), half=False)
    cand = field_rows(2, 333, [(2500, 4000), (4000, 5000)], empty=(9,), half=False)
    dc, dd = dataset(fmhip, ctx), dataset(fmhip, cand)
    got = fm.pairScores(dc, dd)                              # (before the parameters are pulled: the device state is the lazy one)
    idx, sc = fm.recommend(dc, dd, 7)
    S, tol = pair_ref(fm.w0, fm.w, fm.v, ctx, cand)
    assert np.abs(fm.v - a["v"]).max() > 1e-3               # the decay did act
    assert (np.abs(got - S) <= tol).all(), float((np.abs(got - S) / tol).max())
    check_topk(idx, sc, S, tol, 7)
    for d in (ds, dc, dd):
        d.unpersist()
    fm.close()


# ---- 2. fmhip_topk is a valid top-K up to rounding --------------------------------------------------------------------------

def run_topk(fmhip, seed, B, M, k, K, exclude=None, n1=600, rows=None, **kw):
    w0, w, v, ctx, cand = problem(seed, B, M, n1, k, **kw)
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    idx, sc = fm.recommend(dc, dd, K, exclude=exclude)
    assert idx.shape == sc.shape == (B, K) and idx.dtype == np.int32 and sc.dtype == np.float64
    S, tol = pair_ref(w0, w, v, ctx, cand, rows=rows)
    check_topk(idx, sc, S, tol, K, exclude=exclude, contexts=rows)
    dc.unpersist()
    dd.unpersist()
    fm.close()
    return idx, sc


@pytest.mark.parametrize("K", [1, 10, 128])
@pytest.mark.parametrize("k,B,M", [(8, 37, 1003), (64, 70, 5000), (200, 5, 300), (100, 19, 63)])
def test_topk_is_a_valid_top_k(fmhip, K, k, B, M):
    run_topk(fmhip, 3 * K + k, B, M, k, K, empty_c=(1,), empty_d=(2, M - 1))


@pytest.mark.parametrize("K", [1, 10, 128])
def test_topk_with_fewer_candidates_than_k(fmhip, K):
    """M < K: the tail is -1 / -Inf; M = K: every candidate comes back, in order."""
    for M in sorted({max(K - 3, 1), K}):
        idx, sc = run_topk(fmhip, 40 + K, 19, M, 16, K)
        assert (np.sort(idx[:, :min(M, K)], axis=1) == np.arange(min(M, K))).all()


@pytest.mark.parametrize("K", [1, 10, 128])
def test_topk_one_context_many_candidate_splits(fmhip, K):
    run_topk(fmhip, 50 + K, 1, 300000, 32, K, n1=4000)


@pytest.mark.parametrize("K", [1, 10, 128])
def test_topk_many_contexts(fmhip, K):
    run_topk(fmhip, 60 + K, 5000, 2000, 16, K, rows=np.arange(0, 5000, 7))


@pytest.mark.parametrize("K", [1, 10, 128])
def test_topk_exclusion_lists(fmhip, K):
    """Per context: no exclusions, everything excluded, all but K - 1 excluded, a random subset, duplicates and disorder
    (the Python mirror sorts and de-duplicates)."""
    B, M = 23, 700
    rng = np.random.default_rng(K)
    ex = []
    for c in range(B):
        if c % 4 == 0:
            ex.append(np.zeros(0, np.int64))
        elif c % 4 == 1:
            ex.append(np.arange(M))
        elif c % 4 == 2:
            ex.append(rng.permutation(M)[:M - (K - 1)])
        else:
            e = rng.integers(0, M, 300)
            ex.append(np.concatenate([e, e[:50]]))
    idx, sc = run_topk(fmhip, 70 + K, B, M, 24, K, exclude=ex)
    assert (idx[1] == -1).all() and (idx[2, :K - 1] >= 0).all() and idx[2, K - 1] == -1


@pytest.mark.parametrize("K", [1, 10, 128])
def test_topk_catalogue_sorted_by_ascending_score(fmhip, K):
    """The pruning's worst case: the candidates come in ASCENDING score for the context, so every score beats the running
    K-th and is inserted.  One context feature, one candidate feature each: score = const + w_d + x * <v_c, v_d>."""
    k, M, n1 = 8, 3000, 3100
    w0, w, v = params(9, n1, k)
    ctx = dict(row_ptr=np.array([0, 1], np.int64), col=np.array([0], np.int32), val=np.array([1.0]))
    cand = dict(row_ptr=np.arange(M + 1, dtype=np.int64), col=np.arange(10, 10 + M, dtype=np.int32), val=np.ones(M))
    S, _ = pair_ref(w0, w, v, ctx, cand)
    order = np.argsort(S[0], kind="stable")
    cand["col"] = np.ascontiguousarray(cand["col"][order])
    S, tol = pair_ref(w0, w, v, ctx, cand)
    assert (np.diff(S[0]) >= 0).all()
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    idx, sc = fm.recommend(dc, dd, K)
    check_topk(idx, sc, S, tol, K)
    dc.unpersist()
    dd.unpersist()
    fm.close()


# ---- 3. the exact case ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,K", [(4, 1), (8, 10), (8, 128), (3, 32)])
def test_topk_exact_order_with_ties(fmhip, k, K):
    """Small dyadic rationals (V in multiples of 1/4 with |v| <= 1/2, w in multiples of 1/8, x in {1, 1/2}, <= 6 entries per
    joined row): every intermediate is exact in fp32 — asserted here by evaluating the scores in float32 and in float64 numpy —
    and duplicate candidate rows tie on purpose.  idx must be exactly the stable descending argsort of the oracle's scores
    and score must equal them exactly."""
    n1, B, M = 64, 33, 900
    rng = np.random.default_rng(k * 100 + K)
    w0 = 0.25
    w = rng.integers(-4, 5, n1) / 8.0
    v = rng.integers(-2, 3, (k, n1)) / 4.0
    ctx = field_rows(1, B, [(0, 10), (10, 20), (20, 32)], empty=(4,), half=True)
    base = field_rows(2, 60, [(32, 40), (40, 52), (52, 64)], empty=(7,), half=True)
    pick = rng.integers(0, 60, M)                           # 900 candidates drawn from 60 distinct rows: many exact ties
    lens = np.diff(base["row_ptr"])[pick]
    ptr = np.zeros(M + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    sel = np.concatenate([np.arange(base["row_ptr"][p], base["row_ptr"][p + 1]) for p in pick])
    cand = dict(row_ptr=ptr, col=base["col"][sel], val=base["val"][sel])
    S, _ = pair_ref(w0, w, v, ctx, cand)
    # the same expression in float32: exactness of every intermediate shows as equality
    yc, qc, _ = row_stats(w0, w, v, ctx)
    yd, qd, _ = row_stats(w0, w, v, cand)
    dot32 = np.zeros((B, M), np.float32)
    for f in range(k):
        dot32 += qc[:, f].astype(np.float32)[:, None] * qd[:, f].astype(np.float32)[None, :]
    S32 = (yc.astype(np.float32)[:, None] + (yd.astype(np.float32) - np.float32(w0))[None, :]) + dot32
    assert (S32.astype(np.float64) == S).all()
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    np.testing.assert_array_equal(fm.pairScores(dc, dd), S)
    idx, sc = fm.recommend(dc, dd, K)
    want = np.argsort(-S, axis=1, kind="stable")[:, :K]
    np.testing.assert_array_equal(idx, want)
    np.testing.assert_array_equal(sc, np.take_along_axis(S, want, axis=1))
    assert K == 1 or (np.diff(sc, axis=1) == 0).sum() > B   # ties did occur
    assert (np.sort(S, axis=1)[:, -1] == np.sort(S, axis=1)[:, -2]).any()      # ... at the very top, too
    dc.unpersist()
    dd.unpersist()
    fm.close()


# ---- 4. / 5. determinism and consistency --------------------------------------------------------------------------------------

def rows_subset(r, sel):
    lens = np.diff(r["row_ptr"])[sel]
    ptr = np.zeros(len(sel) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    e = np.concatenate([np.arange(r["row_ptr"][p], r["row_ptr"][p + 1]) for p in sel]) if len(sel) else np.zeros(0, np.int64)
    return dict(row_ptr=ptr, col=r["col"][e], val=r["val"][e])


@pytest.mark.parametrize("k", [20, 64])
def test_topk_is_deterministic_and_batch_invariant(fmhip, k):
    """Two calls give identical bytes; a context scored alone gives row i of the batched call bit for bit; permuting the
    contexts permutes the result; the scores are fmhip_pair_scores' at the returned positions, bit for bit; and pair_scores
    agrees with fmhip_predict on explicitly joined rows within 2 tol."""
    n1, B, M, K = 600, 150, 4100, 12
    w0, w, v, ctx, cand = problem(k, B, M, n1, k, empty_c=(5,), empty_d=(6,))
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    idx, sc = fm.recommend(dc, dd, K)
    idx2, sc2 = fm.recommend(dc, dd, K)
    assert idx.tobytes() == idx2.tobytes() and sc.tobytes() == sc2.tobytes()
    for i in (0, 5, 63, 64, 149):
        d1 = dataset(fmhip, rows_subset(ctx, [i]))
        i1, s1 = fm.recommend(d1, dd, K)
        assert i1.tobytes() == idx[i:i + 1].tobytes() and s1.tobytes() == sc[i:i + 1].tobytes(), i
        d1.unpersist()
    perm = np.random.default_rng(0).permutation(B)
    dp = dataset(fmhip, rows_subset(ctx, perm))
    ip, sp = fm.recommend(dp, dd, K)
    assert ip.tobytes() == idx[perm].tobytes() and sp.tobytes() == sc[perm].tobytes()
    full = fm.pairScores(dc, dd)
    assert np.take_along_axis(full, idx.astype(np.int64), axis=1).tobytes() == sc.tobytes()
    # against the parent's route: predict on the joined rows (ids are disjoint: an ordinary row)
    rng = np.random.default_rng(1)
    pairs = [(int(c), int(d)) for c, d in zip(rng.integers(0, B, 3000), rng.integers(0, M, 3000))]
    j = joined(ctx, cand, pairs)
    dj = dataset(fmhip, j)
    yh = fm.predict(dj)
    S, tol = pair_ref(w0, w, v, ctx, cand)
    pc, pd = np.array(pairs).T
    assert (np.abs(yh - full[pc, pd]) <= 2 * tol[pc, pd]).all()
    for d in (dc, dd, dp, dj):
        d.unpersist()
    fm.close()


# ---- 6. NaN / Inf -----------------------------------------------------------------------------------------------------------

def test_topk_ranks_nan_and_inf_as_documented(fmhip):
    """Non-finite parameters: w_J1 = +Inf (a candidate holding J1 scores +Inf), w_J2 = -Inf (-Inf), and a V row holding +Inf
    (feature J3: the candidate's own prediction is Inf - Inf, and 0 * Inf for a context with q_0 = 0: NaN).  +Inf ranks first,
    -Inf after every finite score, NaN after -Inf, ties by row; the other candidates' scores are untouched."""
    n1, k, B, M, K = 300, 8, 40, 500, 10
    w0, w, v, ctx, cand = problem(11, B, M, n1, k, empty_c=(0,))
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    clean = fm.pairScores(dc, dd)
    first = cand["col"][cand["row_ptr"][:-1]]                # (no candidate row is empty here)
    J1, J2, J3 = (int(x) for x in np.unique(first)[:3])
    bad = np.flatnonzero([len(np.intersect1d((J1, J2, J3), cand["col"][cand["row_ptr"][d]:cand["row_ptr"][d + 1]])) > 0 for d in range(M)])
    assert 0 < len(bad) < 100
    w2, v2 = w.copy(), v.copy()
    w2[J1], w2[J2], v2[0, J3] = np.inf, -np.inf, np.inf
    fm.w, fm.v = w2, v2
    full = fm.pairScores(dc, dd)
    good = np.setdiff1d(np.arange(M), bad)
    assert full[:, good].tobytes() == clean[:, good].tobytes()
    assert not np.isfinite(full[:, bad]).any()
    assert np.isposinf(full[:, bad]).any() and np.isneginf(full[:, bad]).any() and np.isnan(full[:, bad]).any()
    idx, sc = fm.recommend(dc, dd, 128)
    for c in range(B):
        key = np.where(np.isnan(full[c]), -np.inf, full[c])
        rank = np.lexsort((np.arange(M), np.isnan(full[c]), -key))       # descending score, NaN after -Inf, ties by row
        np.testing.assert_array_equal(idx[c], rank[:128])
        np.testing.assert_array_equal(sc[c], full[c][rank[:128]])
    # all but a few candidates excluded: the list reaches the -Inf and NaN entries
    keep = np.concatenate([good[:3], bad])
    ex = [np.setdiff1d(np.arange(M), keep)] * B
    idx, sc = fm.recommend(dc, dd, 128, exclude=ex)
    for c in range(B):
        fc = full[c][keep]
        key = np.where(np.isnan(fc), -np.inf, fc)
        rank = keep[np.lexsort((keep, np.isnan(fc), -key))]
        n = min(len(keep), 128)
        np.testing.assert_array_equal(idx[c, :n], rank[:n])
        np.testing.assert_array_equal(sc[c, :n], full[c][rank[:n]])
        assert (idx[c, n:] == -1).all()
    dc.unpersist()
    dd.unpersist()
    fm.close()


# ---- 7. never materialised -----------------------------------------------------------------------------------------------------

@pytest.mark.slow
def test_topk_never_materialises_the_scores(fmhip):
    """200,000 contexts x 1,000,000 candidates, k = 32, K = 10: the B x M scores would be 800 GB (the card has 288 GB).  64
    contexts chosen by a fixed seed pass the valid-top-K check in full.  The call's time limit is 40 x the first measured run
    (0.25 s on an MI355X, 7.8e11 pairs/s; 0.16 s later), so that only a route that materialises or re-gathers exceeds it."""
    B, M, k, K, n1 = 200000, 1000000, 32, 10, 60000
    w0, w, v, ctx, cand = problem(77, B, M, n1, k)
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    t0 = time.perf_counter()
    idx, sc = fm.recommend(dc, dd, K)
    dt = time.perf_counter() - t0
    print("200k x 1M, k=32, K=10: %.2f s, %.3g pairs/s" % (dt, B * M / dt))
    rows = np.sort(np.random.default_rng(2024).choice(B, 64, replace=False))
    S, tol = pair_ref(w0, w, v, ctx, cand, rows=rows)
    check_topk(idx, sc, S, tol, K, contexts=rows)
    assert dt < 10.0, dt
    dc.unpersist()
    dd.unpersist()
    fm.close()


# ---- 8. re-entrancy ------------------------------------------------------------------------------------------------------------

def test_topk_is_reentrant_and_ordered_behind_training(fmhip):
    """Four host threads call recommend on one model at once and each gets the bits a lone caller gets; a training step queued
    on the model's stream (fmhip_sgd_step without stats returns before it has run) is seen by a recommend issued right after."""
    from helpers import random_problem
    from sparkfm_amd import _ffi
    n1, k, B, M, K = 600, 32, 300, 20000, 16
    w0, w, v, ctx, cand = problem(21, B, M, n1, k)
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    lone = fm.recommend(dc, dd, K)
    h = fm.handle
    out, err = [None] * 4, []

    def work(t):
        try:
            for _ in range(3):
                out[t] = fm.recommend(dc, dd, K)
        except Exception as e:       # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    assert not err, err
    for o in out:
        assert o[0].tobytes() == lone[0].tobytes() and o[1].tobytes() == lone[1].tobytes()
    a = random_problem(4, 4000, n1, k, 5, 20)
    tr = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=0).cache()
    _ffi.check(_ffi.load().fmhip_sgd_step(h, tr.handle, 0, 0.5, 0.0, 0.0, 0.0, None))       # asynchronous: no stats, no sync
    after = fm.recommend(dc, dd, K)
    _ffi.check(_ffi.load().fmhip_synchronize(h))
    fm._device_updated()
    settled = fm.recommend(dc, dd, K)
    assert after[1].tobytes() == settled[1].tobytes() and after[0].tobytes() == settled[0].tobytes()
    assert after[1].tobytes() != lone[1].tobytes()
    S, tol = pair_ref(fm.w0, fm.w, fm.v, ctx, cand)
    check_topk(after[0], after[1], S, tol, K)
    for d in (dc, dd, tr):
        d.unpersist()
    fm.close()


# ---- 9. refusals, the C++ mirror -------------------------------------------------------------------------------------------------

def test_topk_refusals(fmhip):
    import ctypes as C
    from sparkfm_amd import _ffi
    L = _ffi.load()
    n1, k = 200, 8
    w0, w, v, ctx, cand = problem(1, 5, 30, n1, k)
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    h, hc, hd = fm.handle, dc.handle, dd.handle
    idx, sc = np.zeros((5, 4), np.int32), np.zeros((5, 4))
    eptr, ex = np.zeros(6, np.int64), np.zeros(4, np.int32)

    def refused(code, text, *args):
        assert L.fmhip_topk(*args) == code, args
        assert text in L.fmhip_last_error().decode(), L.fmhip_last_error()
    P = _ffi.ptr
    refused(-1, "NULL", None, hc, hd, 4, None, None, P(idx), P(sc))
    refused(-1, "NULL", h, None, hd, 4, None, None, P(idx), P(sc))
    refused(-1, "NULL", h, hc, None, 4, None, None, P(idx), P(sc))
    refused(-1, "idx is NULL", h, hc, hd, 4, None, None, None, P(sc))
    refused(-1, "k = 0", h, hc, hd, 0, None, None, P(idx), P(sc))
    refused(-1, "k = 129", h, hc, hd, 129, None, None, P(idx), P(sc))
    refused(-1, "both", h, hc, hd, 4, P(eptr), None, P(idx), P(sc))
    refused(-1, "both", h, hc, hd, 4, None, P(ex), P(idx), P(sc))
    refused(-1, "decreases", h, hc, hd, 4, P(np.array([0, 2, 1, 2, 2, 2], np.int64)), P(ex), P(idx), P(sc))
    refused(-1, "outside", h, hc, hd, 4, P(np.array([0, 1, 1, 1, 1, 1], np.int64)), P(np.array([30], np.int32)), P(idx), P(sc))
    refused(-1, "outside", h, hc, hd, 4, P(np.array([0, 1, 1, 1, 1, 1], np.int64)), P(np.array([-1], np.int32)), P(idx), P(sc))
    refused(-1, "ascending", h, hc, hd, 4, P(np.array([0, 2, 2, 2, 2, 2], np.int64)), P(np.array([7, 7], np.int32)), P(idx), P(sc))
    refused(-1, "ascending", h, hc, hd, 4, P(np.array([0, 2, 2, 2, 2, 2], np.int64)), P(np.array([7, 3], np.int32)), P(idx), P(sc))
    assert L.fmhip_pair_scores(h, hc, hd, 2, 1, P(sc)) == -1 and L.fmhip_pair_scores(h, hc, hd, 0, 6, P(sc)) == -1
    assert L.fmhip_pair_scores(h, hc, hd, 0, 5, None) == -1 and b"out is NULL" in L.fmhip_last_error()
    # a dataset wider than the model: FMHIP_ERR_SHAPE, as the other scoring calls
    wide = dataset(fmhip, dict(row_ptr=np.array([0, 1], np.int64), col=np.array([n1 + 5], np.int32), val=np.ones(1)))
    refused(-4, "num_attribute", h, hc, wide.handle, 4, None, None, P(idx), P(sc))
    refused(-4, "num_attribute", h, wide.handle, hd, 4, None, None, P(idx), P(sc))
    # no contexts / no candidates: not an error
    none = dataset(fmhip, dict(row_ptr=np.zeros(1, np.int64), col=np.zeros(0, np.int32), val=np.zeros(0)))
    assert L.fmhip_topk(h, none.handle, hd, 4, None, None, P(idx), P(sc)) == 0
    idx[:] = 9
    assert L.fmhip_topk(h, hc, none.handle, 4, None, None, P(idx), P(sc)) == 0
    assert (idx == -1).all() and np.isneginf(sc).all()
    assert fm.recommend(none, dd, 3)[0].shape == (0, 3) and fm.pairScores(dc, none).shape == (5, 0)
    # score is optional; the loss and the optimizer do not enter
    i1, s1 = fm.recommend(dc, dd, 4)
    i2, s2 = fm.recommend(dc, dd, 4, scores=False)
    assert s2 is None and i1.tobytes() == i2.tobytes()
    _ffi.check(L.fmhip_model_set_loss(h, _ffi.LOSS_LOGISTIC))
    _ffi.check(L.fmhip_model_set_optimizer(h, _ffi.OPT_ADAGRAD, 1e-8, 0.1))
    i3, s3 = fm.recommend(dc, dd, 4)
    assert i3.tobytes() == i1.tobytes() and s3.tobytes() == s1.tobytes()
    for d in (dc, dd, wide, none):
        d.unpersist()
    fm.close()


def test_cpp_recommend_matches_python(fmhip, tmp_path):
    """include/sparkfm.hpp's FMModel::recommend (tests/cpp_topk.cpp) on a problem both sides build from the same integer
    recipe returns the Python mirror's idx and scores bit for bit."""
    from sparkfm_amd import _build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_topk")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_topk.cpp"), "-L" + _build.LIBDIR, "-lfmhip",
                           "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    lines = [ln.split() for ln in r.stdout.decode().split("\n") if ln.strip()]
    B, M, K, n1, k = 50, 777, 9, 128, 12
    assert len(lines) == B * K
    cpp_idx = np.array([int(ln[0]) for ln in lines], np.int32).reshape(B, K)
    cpp_sc = np.array([float.fromhex(ln[1]) for ln in lines]).reshape(B, K)
    # the recipe of tests/cpp_topk.cpp
    w0 = 0.125
    w = np.array([((i * 7) % 11 - 5) / 32.0 for i in range(n1)])
    v = np.array([[((f * 5 + i * 3) % 13 - 6) / 40.0 for i in range(n1)] for f in range(k)])

    def rows(n, lo, salt):
        ptr, col, val = [0], [], []
        for r in range(n):
            if r % 10 != 3:                                  # (every tenth row is empty)
                for j in range(1 + r % 3):
                    col.append(lo + (r * 5 + j * 17 + salt) % 16 + 16 * j)
                    val.append(1.0 if (r + j) % 2 else 0.5)
            ptr.append(len(col))
        return dict(row_ptr=np.array(ptr, np.int64), col=np.array(col, np.int32), val=np.array(val))
    ctx, cand = rows(B, 0, 1), rows(M, 64, 2)
    ex = [[d for d in range(M) if (d + c) % 5 == 0] for c in range(B)]
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx, scoring=False), dataset(fmhip, cand, scoring=False)
    idx, sc = fm.recommend(dc, dd, K, exclude=ex)
    np.testing.assert_array_equal(cpp_idx, idx)
    assert cpp_sc.tobytes() == sc.tobytes()
    S, tol = pair_ref(w0, w, v, ctx, cand)
    check_topk(idx, sc, S, tol, K, exclude=ex)
    dc.unpersist()
    dd.unpersist()
    fm.close()
