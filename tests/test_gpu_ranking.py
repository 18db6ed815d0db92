"""GPU checks of ranking evaluation (include/fmhip_ranking.h: fmhip_rank; FMModel.rankOf / computeRankingMetrics).

The yardstick is exact — no tolerance, no exemptions: numpy ranks the bits fm.pairScores returns (tests/rank_ref.py: ranks_of),
    rank = #{d not excluded, d != t: S[d] > S[t] or (S[d] == S[t] and d < t)},   NaN below -inf, NaNs by row,
and pairScores is held to the fp64 oracle by tests/test_gpu_topk.py.  Every returned score must be S[c, t] bit for bit."""
import os
import subprocess
import threading
import time

import numpy as np
import pytest

from rank_ref import FIELDS, rank_ref, ranks_of
from topk_ref import field_rows, pair_ref, params

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
    """contexts over ids [0, n1/2), candidates over [n1/2, n1): three fields a side (as tests/test_gpu_topk.py)"""
    h = n1 // 2
    w0, w, v = params(seed, n1, k, scale)
    ctx = field_rows(seed + 100, B, [(0, h // 2), (h // 2, h - 8), (h - 8, h)], empty=empty_c, half=False)
    cand = field_rows(seed + 200, M, [(h, h + h // 2), (h + h // 2, n1 - 8), (n1 - 8, n1)], empty=empty_d, half=False)
    return w0, w, v, ctx, cand


def relevant_rows(seed, B, M, most=3):
    """0 .. most distinct rows per context, unsorted"""
    rng = np.random.default_rng(seed)
    return [rng.choice(M, int(rng.integers(0, most + 1)), replace=False) for _ in range(B)]


def check_ranks(ranks, scores, S, relevant, exclude=None, contexts=None):
    """every rank is numpy's rank of the bits in S, every score S's own bits; S's rows stand for `contexts`"""
    rows = range(S.shape[0]) if contexts is None else contexts
    for si, c in enumerate(rows):
        t = np.unique(np.asarray(relevant[c], np.int64))
        want = ranks_of(S[si], t, None if exclude is None else exclude[c])
        assert ranks[c].dtype == np.int32 and ranks[c].shape == (len(t),), (c, ranks[c])
        np.testing.assert_array_equal(ranks[c], want, err_msg="context %d" % c)
        if scores is not None:
            assert scores[c].tobytes() == S[si, t].tobytes(), (c, scores[c], S[si, t])


def rows_subset(r, sel):
    lens = np.diff(r["row_ptr"])[sel]
    ptr = np.zeros(len(sel) + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    e = np.concatenate([np.arange(r["row_ptr"][p], r["row_ptr"][p + 1]) for p in sel]) if len(sel) else np.zeros(0, np.int64)
    return dict(row_ptr=ptr, col=r["col"][e], val=r["val"][e])


# ---- 1. every rank and every score, all four padded widths ---------------------------------------------------------------------

@pytest.mark.parametrize("k,B,M", [(8, 37, 1003), (33, 70, 5000), (100, 19, 63), (200, 5, 300)])
def test_ranks_are_numpy_ranks_of_the_pair_scores(fmhip, k, B, M):
    """Kp = 32, 64, 128, 256; the query count and M off every multiple of 16 and 64; 0-3 relevant rows per context, one context
    without any; an empty context row that has relevant rows; empty candidate rows (they tie with each other exactly) among the
    relevant ones.  The contexts' dataset is cut into batches of 16 rows, so chunks cut rel_ptr mid-array — and once more as
    one batch, so that (B = 70) one sweep holds more than 64 queries."""
    w0, w, v, ctx, cand = problem(k, B, M, 600, k, empty_c=(1,), empty_d=(2, M - 1))
    rel = relevant_rows(k, B, M)
    rel[0], rel[1], rel[3] = np.array([M - 1, 2, 5]), np.array([7, 2]), np.zeros(0, np.int64)
    fm, dd = model(fmhip, 600, k, w0, w, v), dataset(fmhip, cand)
    for batch_rows in (16, 0):
        dc = dataset(fmhip, ctx, scoring=False, batch_rows=batch_rows)
        S = fm.pairScores(dc, dd)
        ranks, scores = fm.rankOf(dc, dd, rel, scores=True)
        assert len(ranks) == len(scores) == B and len(ranks[3]) == 0
        check_ranks(ranks, scores, S, rel)
        only = fm.rankOf(dc, dd, rel)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(only, ranks))
        dc.unpersist()
    dd.unpersist()
    fm.close()


def test_rank_one_query_many_candidate_splits(fmhip):
    """one context x 300,000 candidates, k = 32: the one query block is cut into hundreds of candidate splits"""
    M = 300000
    w0, w, v, ctx, cand = problem(50, 1, M, 4000, 32)
    fm, dc, dd = model(fmhip, 4000, 32, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    S = fm.pairScores(dc, dd)                      # one row
    best, worst = int(np.argmax(S[0])), int(np.argmin(S[0]))
    rel = [np.array([123456, best, worst, 0, M - 1])]
    ranks, scores = fm.rankOf(dc, dd, rel, scores=True)
    check_ranks(ranks, scores, S, rel)
    t = np.unique(rel[0])
    assert ranks[0][t == best][0] == 0 and ranks[0][t == worst][0] == M - 1
    dc.unpersist()
    dd.unpersist()
    fm.close()


# ---- 2. exclusions --------------------------------------------------------------------------------------------------------------

def test_rank_exclusion_lists(fmhip):
    """Per context: no exclusions, all but the relevant rows, a random 300 of 700 (some beat the target, some do not; with
    duplicates and disorder: the Python mirror sorts and de-duplicates).  A row both relevant and excluded is refused by the
    C ABI and by Python."""
    from sparkfm_amd import _ffi
    B, M, k = 23, 700, 24
    w0, w, v, ctx, cand = problem(70, B, M, 600, k)
    rng = np.random.default_rng(5)
    rel = [rng.choice(M, int(rng.integers(1, 4)), replace=False) for _ in range(B)]
    ex = []
    for c in range(B):
        others = np.setdiff1d(np.arange(M), rel[c])
        if c % 3 == 0:
            ex.append(np.zeros(0, np.int64))
        elif c % 3 == 1:
            ex.append(others)
        else:
            e = rng.permutation(others)[:300]
            ex.append(np.concatenate([e, e[:50]]))
    fm, dc, dd = model(fmhip, 600, k, w0, w, v), dataset(fmhip, ctx, scoring=False, batch_rows=6), dataset(fmhip, cand)
    S = fm.pairScores(dc, dd)
    ranks, scores = fm.rankOf(dc, dd, rel, exclude=ex, scores=True)
    check_ranks(ranks, scores, S, rel, exclude=ex)
    plain = fm.rankOf(dc, dd, rel)
    for c in range(B):
        t = np.unique(rel[c])
        if c % 3 == 1:           # only the relevant rows are left: they rank among themselves
            np.testing.assert_array_equal(np.sort(ranks[c]), np.arange(len(t)))
        if c % 3 == 2:           # some of the excluded rows beat the target, some do not
            beat = [(S[c, np.unique(ex[c])] > S[c, x]).sum() for x in t]
            assert all(0 < b < 300 for b in beat) or len(t) == 0, (c, beat)
            np.testing.assert_array_equal(plain[c] - ranks[c], beat)
    # relevant and excluded: refused through both
    bad = [e.copy() for e in ex]
    bad[5] = np.append(bad[5], rel[5][0])
    with pytest.raises(ValueError, match="both relevant and excluded for context 5"):
        fm.rankOf(dc, dd, rel, exclude=bad)
    rptr, ridx = _ffi.row_lists(rel, B, M, "relevant")
    eptr, eidx = _ffi.row_lists(bad, B, M, "exclude")
    out = np.zeros(int(rptr[B]), np.int32)
    L = _ffi.load()
    args = (fm.handle, dc.handle, dd.handle, _ffi.ptr(rptr), _ffi.ptr(ridx), _ffi.ptr(eptr), _ffi.ptr(eidx), _ffi.ptr(out), None)
    assert L.fmhip_rank(*args) == -1
    assert "both relevant and excluded for context 5" in L.fmhip_last_error().decode()
    dc.unpersist()
    dd.unpersist()
    fm.close()


def test_rank_refusals(fmhip):
    """fmhip_topk's refusals, and fmhip_rank's own; what is not an error."""
    from sparkfm_amd import _ffi
    L = _ffi.load()
    n1, k = 200, 8
    w0, w, v, ctx, cand = problem(1, 5, 30, n1, k)
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    h, hc, hd = fm.handle, dc.handle, dd.handle
    P = _ffi.ptr
    rptr, rel = np.array([0, 1, 1, 3, 3, 3], np.int64), np.array([4, 0, 29], np.int32)
    eptr, ex = np.zeros(6, np.int64), np.zeros(4, np.int32)
    rank, sc = np.full(3, -7, np.int32), np.zeros(3)

    def refused(code, text, *args):
        assert L.fmhip_rank(*args) == code, args
        assert text in L.fmhip_last_error().decode(), L.fmhip_last_error()
    i64 = lambda *a: P(np.array(a, np.int64))       # noqa: E731
    i32 = lambda *a: P(np.array(a, np.int32))       # noqa: E731
    refused(-1, "NULL", None, hc, hd, P(rptr), P(rel), None, None, P(rank), P(sc))
    refused(-1, "NULL", h, None, hd, P(rptr), P(rel), None, None, P(rank), P(sc))
    refused(-1, "NULL", h, hc, None, P(rptr), P(rel), None, None, P(rank), P(sc))
    refused(-1, "rel_ptr is NULL", h, hc, hd, None, P(rel), None, None, P(rank), P(sc))
    refused(-1, "rel or rank is NULL", h, hc, hd, P(rptr), None, None, None, P(rank), P(sc))
    refused(-1, "rel or rank is NULL", h, hc, hd, P(rptr), P(rel), None, None, None, P(sc))
    refused(-1, "rel_ptr[0] < 0", h, hc, hd, i64(-1, 1, 1, 3, 3, 3), P(rel), None, None, P(rank), P(sc))
    refused(-1, "rel_ptr decreases at context 1", h, hc, hd, i64(0, 2, 1, 3, 3, 3), P(rel), None, None, P(rank), P(sc))
    refused(-1, "outside [0, 30)", h, hc, hd, P(rptr), i32(4, 0, 30), None, None, P(rank), P(sc))
    refused(-1, "outside [0, 30)", h, hc, hd, P(rptr), i32(-1, 0, 29), None, None, P(rank), P(sc))
    refused(-1, "relevant rows of context 2 are not ascending", h, hc, hd, P(rptr), i32(4, 9, 9), None, None, P(rank), P(sc))
    refused(-1, "relevant rows of context 2 are not ascending", h, hc, hd, P(rptr), i32(4, 9, 3), None, None, P(rank), P(sc))
    refused(-1, "both", h, hc, hd, P(rptr), P(rel), P(eptr), None, P(rank), P(sc))
    refused(-1, "both", h, hc, hd, P(rptr), P(rel), None, P(ex), P(rank), P(sc))
    refused(-1, "decreases", h, hc, hd, P(rptr), P(rel), i64(0, 2, 1, 2, 2, 2), P(ex), P(rank), P(sc))
    refused(-1, "outside", h, hc, hd, P(rptr), P(rel), i64(0, 1, 1, 1, 1, 1), i32(30), P(rank), P(sc))
    refused(-1, "ascending", h, hc, hd, P(rptr), P(rel), i64(0, 2, 2, 2, 2, 2), i32(7, 7), P(rank), P(sc))
    refused(-1, "both relevant and excluded for context 2", h, hc, hd, P(rptr), P(rel), i64(0, 0, 0, 2, 2, 2), i32(3, 29), P(rank), P(sc))
    assert (rank == -7).all()
    wide = dataset(fmhip, dict(row_ptr=np.array([0, 1], np.int64), col=np.array([n1 + 5], np.int32), val=np.ones(1)))
    refused(-4, "num_attribute", h, hc, wide.handle, i64(0, 0, 0, 0, 0, 0), P(rel), None, None, P(rank), P(sc))
    refused(-4, "num_attribute", h, wide.handle, hd, i64(0, 0), P(rel), None, None, P(rank), P(sc))
    # not errors: no contexts (rel_ptr may then be NULL), no relevant rows (rel and rank may be NULL), no candidates and no relevant rows
    none = dataset(fmhip, dict(row_ptr=np.zeros(1, np.int64), col=np.zeros(0, np.int32), val=np.zeros(0)))
    assert L.fmhip_rank(h, none.handle, hd, None, None, None, None, None, None) == 0
    assert L.fmhip_rank(h, hc, hd, P(np.zeros(6, np.int64)), None, None, None, None, None) == 0
    assert L.fmhip_rank(h, hc, none.handle, P(np.zeros(6, np.int64)), None, None, None, None, None) == 0
    refused(-1, "outside [0, 0)", h, hc, none.handle, P(rptr), P(rel), None, None, P(rank), P(sc))
    assert fm.rankOf(none, dd, []) == [] and [len(r) for r in fm.rankOf(dc, dd, [[]] * 5)] == [0] * 5
    # offsets that start above 0 index rel, rank and score as they stand; the loss and the optimizer do not enter
    assert L.fmhip_rank(h, hc, hd, P(rptr), P(rel), None, None, P(rank), P(sc)) == 0
    r2, s2 = np.full(5, -7, np.int32), np.full(5, -7.0)
    _ffi.check(L.fmhip_model_set_loss(h, _ffi.LOSS_LOGISTIC))
    _ffi.check(L.fmhip_model_set_optimizer(h, _ffi.OPT_ADAGRAD, 1e-8, 0.1))
    assert L.fmhip_rank(h, hc, hd, P(rptr + 2), i32(-9, -9, 4, 0, 29), None, None, P(r2), P(s2)) == 0
    assert (r2[:2] == -7).all() and r2[2:].tobytes() == rank.tobytes() and s2[2:].tobytes() == sc.tobytes()
    S = fm.pairScores(dc, dd)
    check_ranks([rank[0:1], rank[1:1], rank[1:3], rank[3:3], rank[3:3]], None, S, [[4], [], [0, 29], [], []])
    for d in (dc, dd, wide, none):
        d.unpersist()
    fm.close()


# ---- 3. the exact case -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [4, 8, 3])
def test_rank_exact_order_with_ties(fmhip, k):
    """The case of test_topk_exact_order_with_ties: small dyadic rationals, every intermediate exact in fp32, 900 candidates drawn
    from 60 distinct rows, so most scores tie with a dozen others.  For three contexts (one an empty row) EVERY candidate is
    relevant: their ranks must be the inverse of the stable descending argsort of the ORACLE's fp64 scores; the other
    contexts hold a few relevant rows each."""
    n1, B, M = 64, 33, 900
    rng = np.random.default_rng(k * 100)
    w0 = 0.25
    w = rng.integers(-4, 5, n1) / 8.0
    v = rng.integers(-2, 3, (k, n1)) / 4.0
    ctx = field_rows(1, B, [(0, 10), (10, 20), (20, 32)], empty=(4,), half=True)
    base = field_rows(2, 60, [(32, 40), (40, 52), (52, 64)], empty=(7,), half=True)
    pick = rng.integers(0, 60, M)
    lens = np.diff(base["row_ptr"])[pick]
    ptr = np.zeros(M + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    sel = np.concatenate([np.arange(base["row_ptr"][p], base["row_ptr"][p + 1]) for p in pick])
    cand = dict(row_ptr=ptr, col=base["col"][sel], val=base["val"][sel])
    S, _ = pair_ref(w0, w, v, ctx, cand)                      # the oracle's, fp64
    rel = relevant_rows(k, B, M)
    for c in (0, 4, 20):
        rel[c] = np.arange(M)
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    np.testing.assert_array_equal(fm.pairScores(dc, dd), S)  # exact: the device's bits are the oracle's values
    ranks, scores = fm.rankOf(dc, dd, rel, scores=True)
    for c in (0, 4, 20):
        order = np.argsort(-S[c], kind="stable")
        inverse = np.empty(M, np.int64)
        inverse[order] = np.arange(M)
        np.testing.assert_array_equal(ranks[c], inverse)
        np.testing.assert_array_equal(scores[c], S[c])
        assert len(np.unique(S[c])) < M // 4                  # ties did occur
    check_ranks(ranks, scores, S, rel)
    dc.unpersist()
    dd.unpersist()
    fm.close()


# ---- 4. consistency with recommend ---------------------------------------------------------------------------------------------

def test_rank_agrees_with_recommend(fmhip):
    """K = 128: rank[p] < K <=> idx[c, rank[p]] == rel[p], and the scores are the list's bit for bit — without and with exclusions."""
    B, M, k, K = 45, 1500, 20, 128
    w0, w, v, ctx, cand = problem(31, B, M, 600, k, empty_c=(2,), empty_d=(3,))
    fm, dc, dd = model(fmhip, 600, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    rng = np.random.default_rng(3)
    for exclude in (None, [rng.choice(M, 400, replace=False) for _ in range(B)]):
        idx, sc = fm.recommend(dc, dd, K, exclude=exclude)
        # half of the relevant rows from the list itself, half from anywhere (not excluded)
        rel = []
        for c in range(B):
            free = np.arange(M) if exclude is None else np.setdiff1d(np.arange(M), exclude[c])
            rel.append(np.unique(np.concatenate([idx[c, rng.integers(0, K, 4)], rng.choice(free, 4, replace=False)])))
        ranks, scores = fm.rankOf(dc, dd, rel, exclude=exclude, scores=True)
        inside = 0
        for c in range(B):
            for t, r, s in zip(rel[c], ranks[c], scores[c]):
                assert (r < K) == (t in idx[c]), (c, t, r)
                if r < K:
                    assert idx[c, r] == t and sc[c, r].tobytes() == s.tobytes(), (c, t, r)
                    inside += 1
        assert inside >= 4 * B - B
    dc.unpersist()
    dd.unpersist()
    fm.close()


# ---- 5. NaN / Inf -----------------------------------------------------------------------------------------------------------------

def test_rank_places_nan_and_inf_as_documented(fmhip):
    """The construction of test_topk_ranks_nan_and_inf_as_documented: w_J1 = +Inf, w_J2 = -Inf, a V row holding +Inf.  Every
    candidate with a non-finite score and a few finite ones are relevant: +Inf ranks first, -Inf after every finite score, NaN
    after -Inf, equal scores and NaNs by row."""
    n1, k, B, M = 300, 8, 40, 500
    w0, w, v, ctx, cand = problem(11, B, M, n1, k, empty_c=(0,))
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    first = cand["col"][cand["row_ptr"][:-1]]
    J1, J2, J3 = (int(x) for x in np.unique(first)[:3])
    bad = np.flatnonzero([len(np.intersect1d((J1, J2, J3), cand["col"][cand["row_ptr"][d]:cand["row_ptr"][d + 1]])) > 0 for d in range(M)])
    good = np.setdiff1d(np.arange(M), bad)
    w2, v2 = w.copy(), v.copy()
    w2[J1], w2[J2], v2[0, J3] = np.inf, -np.inf, np.inf
    fm.w, fm.v = w2, v2
    full = fm.pairScores(dc, dd)
    assert np.isposinf(full[:, bad]).any() and np.isneginf(full[:, bad]).any() and np.isnan(full[:, bad]).any()
    rel = [np.concatenate([bad, good[:5]])] * B
    ranks, scores = fm.rankOf(dc, dd, rel, scores=True)
    check_ranks(ranks, scores, full, rel)
    ex = [good[5:200]] * B
    ranks_ex, _ = fm.rankOf(dc, dd, rel, exclude=ex, scores=True)
    check_ranks(ranks_ex, None, full, rel, exclude=ex)
    for c in range(B):
        t = np.unique(rel[c])
        key = np.where(np.isnan(full[c]), -np.inf, full[c])
        order = np.lexsort((np.arange(M), np.isnan(full[c]), -key))       # descending score, NaN after -Inf, ties by row
        inverse = np.empty(M, np.int64)
        inverse[order] = np.arange(M)
        np.testing.assert_array_equal(ranks[c], inverse[t])
        s = full[c, t]
        n_inf, n_nan, n_ninf = int(np.isposinf(full[c]).sum()), int(np.isnan(full[c]).sum()), int(np.isneginf(full[c]).sum())
        assert (ranks[c][np.isposinf(s)] < n_inf).all() and (ranks[c][np.isnan(s)] >= M - n_nan).all()
        assert ((ranks[c][np.isneginf(s)] >= M - n_nan - n_ninf) & (ranks[c][np.isneginf(s)] < M - n_nan)).all()
        assert (np.diff(ranks[c][np.isnan(s)]) > 0).all()                  # NaNs among themselves: by row
    dc.unpersist()
    dd.unpersist()
    fm.close()


# ---- 6. determinism ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [20, 64])
def test_rank_is_deterministic_and_batch_invariant(fmhip, k):
    """Two calls give identical bytes; a context ranked alone gets the ranks and scores it gets inside the batch; the contexts'
    batch_rows changes nothing (training datasets without the dense hot block: with it the FORWARD sums a row in an order that
    depends on the batch's hot features — tests/test_gpu_topk.py says the same of pairScores — which is not the chunking's doing)."""
    n1, B, M = 600, 150, 4100
    w0, w, v, ctx, cand = problem(k, B, M, n1, k, empty_c=(5,), empty_d=(6,))
    rel = relevant_rows(k + 1, B, M)
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    ranks, scores = fm.rankOf(dc, dd, rel, scores=True)
    again = fm.rankOf(dc, dd, rel, scores=True)
    flat = lambda x: np.concatenate(x).tobytes()       # noqa: E731
    assert flat(ranks) == flat(again[0]) and flat(scores) == flat(again[1])
    check_ranks(ranks, scores, fm.pairScores(dc, dd), rel)
    for i in (0, 5, 63, 64, 149):
        d1 = dataset(fmhip, rows_subset(ctx, [i]))
        r1, s1 = fm.rankOf(d1, dd, [rel[i]], scores=True)
        assert r1[0].tobytes() == ranks[i].tobytes() and s1[0].tobytes() == scores[i].tobytes(), i
        d1.unpersist()
    for batch_rows in (16, 50, 0):
        db = fmhip.DataSet(ctx["row_ptr"], ctx["col"], ctx["val"], np.zeros(B), batch_rows=batch_rows, hot_block=False).cache()
        rb, sb = fm.rankOf(db, dd, rel, scores=True)
        check_ranks(rb, sb, fm.pairScores(db, dd), rel)
        if batch_rows == 16:
            first = (rb, sb)
        assert flat(rb) == flat(first[0]) and flat(sb) == flat(first[1]), batch_rows
        db.unpersist()
    dc.unpersist()
    dd.unpersist()
    fm.close()


# ---- 7. a lazily decayed model ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [16, 32])
def test_rank_of_a_lazily_decayed_model(fmhip, k):
    """After rows-only updates with weight decay (regv > 0) the model holds V = sv * U with sv != 1: the ranks are those of the
    scores pairScores reports for the same device state."""
    from helpers import random_problem
    a = random_problem(5, 300, 5000, k, 2, 8)
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=100).cache()
    fm = model(fmhip, a["n1"], k, a["w0"], a["w"], a["v"])
    sgd = fmhip.HipSGD(eta=0.5, reg0=0.0, regw=0.2, regv=0.2)
    sgd.learn(fm, ds)
    ctx = field_rows(1, 21, [(0, 1000), (1000, 2500)], empty=(3,), half=False)
    cand = field_rows(2, 333, [(2500, 4000), (4000, 5000)], empty=(9,), half=False)
    dc, dd = dataset(fmhip, ctx), dataset(fmhip, cand)
    rel = relevant_rows(k, 21, 333)
    ranks, scores = fm.rankOf(dc, dd, rel, scores=True)      # (before the parameters are pulled: the device state is the lazy one)
    S = fm.pairScores(dc, dd)
    check_ranks(ranks, scores, S, rel)
    assert np.abs(fm.v - a["v"]).max() > 1e-3               # the decay did act
    for d in (ds, dc, dd):
        d.unpersist()
    fm.close()


# ---- 8. the metrics, the C++ mirror ----------------------------------------------------------------------------------------------

def test_compute_ranking_metrics(fmhip):
    from sparkfm_amd import metrics
    B, M, k = 60, 800, 12
    w0, w, v, ctx, cand = problem(41, B, M, 600, k)
    rel = relevant_rows(9, B, M, most=5)
    ex = [np.setdiff1d(np.arange(c % 7, M, 7), rel[c]) for c in range(B)]
    fm, dc, dd = model(fmhip, 600, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    for K in (1, 10, 200):
        got = fm.computeRankingMetrics(dc, dd, rel, k=K, exclude=ex)
        ranks = fm.rankOf(dc, dd, rel, exclude=ex)
        assert got == metrics.ranking_metrics(ranks, K)
        want = rank_ref(ranks, K)
        assert all(got[f] == want[f] for f in ("k", "contexts", "skipped", "relevant"))
        assert all(abs(got[f] - want[f]) <= 1e-13 * abs(want[f]) for f in FIELDS), (got, want)       # (tests/test_host_ranking.py: RTOL)
        assert got["skipped"] == sum(len(r) == 0 for r in rel) > 0 and 0 < got["mrr"] < 1
    assert fm.computeRankingMetrics(dc, dd, rel)["k"] == 10
    dc.unpersist()
    dd.unpersist()
    fm.close()


def test_cpp_rank_matches_python(fmhip, tmp_path):
    """include/sparkfm.hpp's FMModel::rankOf / computeRankingMetrics (tests/cpp_ranking.cpp) on a problem both sides build from
    the same integer recipe: the Python mirror's ranks, scores and metrics bit for bit."""
    from sparkfm_amd import _build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_ranking")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_ranking.cpp"), "-L" + _build.LIBDIR, "-lfmhip",
                           "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    lines = [ln.split() for ln in r.stdout.decode().split("\n") if ln.strip()]
    B, M, K, n1, k = 50, 777, 9, 128, 12
    # the recipe of tests/cpp_ranking.cpp
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
    rel = [sorted({(c * 7) % M, (c * 7 + 300) % M}) if c % 6 else [] for c in range(B)]
    ex = [[d for d in range(M) if (d + c) % 5 == 0 and d not in rel[c]] for c in range(B)]
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx, scoring=False, batch_rows=16), dataset(fmhip, cand, scoring=False)
    ranks, scores = fm.rankOf(dc, dd, rel, exclude=ex, scores=True)
    n = sum(len(r) for r in rel)
    assert len(lines) == n + 1
    assert [int(ln[0]) for ln in lines[:n]] == np.concatenate(ranks).tolist()
    assert np.array([float.fromhex(ln[1]) for ln in lines[:n]]).tobytes() == np.concatenate(scores).tobytes()
    got = fm.computeRankingMetrics(dc, dd, rel, k=K, exclude=ex)
    last = lines[n]
    assert [int(x) for x in last[:3]] == [got["contexts"], got["skipped"], got["relevant"]]
    assert [float.fromhex(x) for x in last[3:]] == [got[f] for f in FIELDS]
    check_ranks(ranks, scores, fm.pairScores(dc, dd), rel, exclude=ex)
    dc.unpersist()
    dd.unpersist()
    fm.close()


# ---- 9. re-entrancy ---------------------------------------------------------------------------------------------------------------

def test_rank_is_reentrant_beside_training(fmhip):
    """Four host threads call rankOf on one model: each gets the bytes a lone caller gets.  Then the same beside a fifth thread
    that trains the model, three steps: a scoring call holds the model's lock shared, so it sees the parameters of before or
    after a step, never of the middle of one — every answer is the serial answer of ONE of the four parameter states (numpy's
    ranks of the pairScores the training thread fetches between its steps).  A step queued without a synchronisation is seen
    by the rankOf issued right after."""
    from helpers import random_problem
    from sparkfm_amd import _ffi
    n1, k, B, M = 600, 32, 300, 20000
    w0, w, v, ctx, cand = problem(21, B, M, n1, k)
    rel = relevant_rows(2, B, M)
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    a = random_problem(4, 4000, n1, k, 5, 20)
    tr = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=0).cache()
    L, h = _ffi.load(), fm.handle
    flat = lambda x: np.concatenate(x[0]).tobytes() + np.concatenate(x[1]).tobytes()       # noqa: E731

    def serial(S):
        t = [np.unique(r) for r in rel]
        return flat(([ranks_of(S[c], t[c]) for c in range(B)], [S[c, t[c]] for c in range(B)]))
    states = [serial(fm.pairScores(dc, dd))]
    assert flat(fm.rankOf(dc, dd, rel, scores=True)) == states[0]
    out, err = [[] for _ in range(4)], []

    def work(t):
        try:
            for _ in range(3):
                out[t].append(flat(fm.rankOf(dc, dd, rel, scores=True)))
        except Exception as e:       # noqa: BLE001
            err.append(e)

    def train():
        try:
            for _ in range(3):
                _ffi.check(L.fmhip_sgd_step(h, tr.handle, 0, 0.5, 0.0, 0.0, 0.0, None))       # asynchronous: no stats, no sync
                states.append(serial(fm.pairScores(dc, dd)))       # (nobody else steps: the state every later call sees)
        except Exception as e:       # noqa: BLE001
            err.append(e)
    th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    assert not err, err
    assert all(len(res) == 3 and o == states[0] for res in out for o in res)
    out = [[] for _ in range(4)]
    th = [threading.Thread(target=work, args=(t,)) for t in range(4)] + [threading.Thread(target=train)]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    assert not err, err
    assert len(states) == 4 and len(set(states)) == 4                 # the steps did change the ranking
    assert all(len(res) == 3 and o in states for res in out for o in res)
    assert flat(fm.rankOf(dc, dd, rel, scores=True)) == states[3]
    # a step queued on the model's stream is seen by the rankOf issued right after
    _ffi.check(L.fmhip_sgd_step(h, tr.handle, 0, 0.5, 0.0, 0.0, 0.0, None))
    after = flat(fm.rankOf(dc, dd, rel, scores=True))
    _ffi.check(L.fmhip_synchronize(h))
    fm._device_updated()
    assert after == flat(fm.rankOf(dc, dd, rel, scores=True)) and after not in states
    for d in (dc, dd, tr):
        d.unpersist()
    fm.close()


# ---- 10. never materialised ----------------------------------------------------------------------------------------------------------

@pytest.mark.slow
def test_rank_never_materialises_the_scores(fmhip):
    """256 queries x 2,000,000 candidates, k = 32: the scores would be 2 GB as floats.  The device memory in use is sampled while
    the call runs: its peak rise stays below a quarter of that (the candidates' q table is 256 MB, everything else a few MB).
    16 queries chosen by a fixed seed are checked against pairScores."""
    import torch
    B, M, k, n1 = 256, 2000000, 32, 60000
    w0, w, v, ctx, cand = problem(78, B, M, n1, k)
    fm, dc, dd = model(fmhip, n1, k, w0, w, v), dataset(fmhip, ctx), dataset(fmhip, cand)
    rel = [np.array([int(x)]) for x in np.random.default_rng(8).integers(0, M, B)]
    fm.rankOf(dc, dd, rel)                                    # (streams, workspace pool: made once)

    def used():
        free, total = torch.cuda.mem_get_info()
        return total - free
    before, peak, stop = used(), [0], threading.Event()

    def watch():
        while not stop.is_set():
            peak[0] = max(peak[0], used())
            time.sleep(0.0005)
    th = threading.Thread(target=watch)
    th.start()
    t0 = time.perf_counter()
    ranks, scores = fm.rankOf(dc, dd, rel, scores=True)
    dt = time.perf_counter() - t0
    stop.set()
    th.join()
    rise = peak[0] - before
    print("256 x 2M, k=32: %.3f s, %.3g pairs/s, peak rise %.0f MB of %.0f MB" % (dt, B * M / dt, rise / 2 ** 20, B * M * 4 / 2 ** 20))
    assert 0 < rise < B * M * 4 // 4, rise
    rows = np.sort(np.random.default_rng(2024).choice(B, 16, replace=False))
    for c in rows:
        S = fm.pairScores(dc, dd, c, c + 1)
        check_ranks(ranks, scores, S, rel, contexts=[c])
    dc.unpersist()
    dd.unpersist()
    fm.close()
