"""Adaptive negatives of the BPR trainer on the GPU (include/fmhip_bpr_adaptive.h) against the fp64 twin of bpr_adaptive_ref.py: the
candidates bit for bit, their scores to the project's pair tolerance, the kept row against the first strict maximum of the device's
own scores and — on a dyadic model where fp32 is exact and ties are planted — against the twin's, n_candidates = 1 against the
uniform trainer, the epoch against resample + steps, the margins, two planted tasks, the refusals and include/sparkfm.hpp.

The base shape is bpr_ref.make_problem's 40 contexts x 120 items with 599 interactions: 599 pairs are no multiple of the pairs a
wave (8, 4, 2, 1) or a block (32, 16, 8, 4) serves at any row width, so the last wave always holds groups without a pair."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bpr_adaptive_ref as aref
import bpr_ref as bref
from test_gpu_adagrad import EPS, get_state
from topk_ref import field_rows
from train_ref import same

pytestmark = pytest.mark.gpu

REGS = (1e-3, 2e-3, 3e-3)
ETA = 0.05
CUT = 256
N_INTER = 599


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


def close(bpr, fm=None):
    bpr.close()
    bpr.contexts.unpersist()
    bpr.candidates.unpersist()
    if fm is not None:
        fm.close()


def forced_positives(seed, n_ctx=40, M=120, n_inter=N_INTER):
    """The base problem's shape with context 0 holding 119 of the 120 rows (all but row 77)."""
    rng = np.random.default_rng(seed)
    flat = rng.choice((n_ctx - 1) * M, size=n_inter - (M - 1), replace=False)
    return [np.setdiff1d(np.arange(M), [77])] + [np.sort(flat[flat // M == u] % M) for u in range(n_ctx - 1)]


def problem(case, k=8, seed=30):
    if case == "forced":
        return bref.make_problem(seed + 1, k, n_inter=N_INTER, positives=forced_positives(seed + 1))
    if case == "two_rows":
        return bref.make_problem(seed + 2, k, n_ctx=9, M=2, n_neg=3, positives=[[u % 2] if u % 3 else [] for u in range(9)])
    return bref.make_problem(seed, k, n_inter=N_INTER)


def twin_draw(P, t, C):
    return aref.draw(P, t, C, P["w0"], P["w"], P["v"])


# ---- 1. the candidates ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["base", "forced", "two_rows"])
def test_candidates_equal_the_twin(fmhip, case):
    """candidate_draws' rows for C in {1, 2, 5, 64} and t in {0, 7} against the twin's, bit for bit, and the attempts / forced of
    resample(t, fm) against the twin's sums over all candidates — on the base problem, with a context that holds 119 of 120 rows
    (every candidate of its pairs is row 77, most of them forced) and on a 2-row candidates block."""
    P = problem(case)
    ctx = np.repeat(P["ctx"], P["n_neg"])
    assert case == "two_rows" or len(ctx) == N_INTER
    for n_cand in (1, 2, 5, 64):
        bpr, fm = bref.build(fmhip, P, batch_pairs=128, n_candidates=n_cand)
        assert bpr.n_candidates == n_cand
        for t in (0, 7):
            want, attempts, forced = aref.candidates(P["seed"], t, ctx, P["ptr"], P["rows"], P["M"], n_cand)
            rows, scores = bpr.candidate_draws(fm, t)
            assert rows.dtype == np.int32 and rows.shape == (len(ctx), n_cand) and np.array_equal(rows, want)
            assert scores.dtype == np.float32 and scores.shape == rows.shape and np.isfinite(scores).all()
            assert np.array_equal(rows[:, 0], bref.draw(P, t)[0])                       # candidate 0 is the uniform draw
            p1 = min(38, len(ctx))
            sub = bpr.candidate_draws(fm, t, 5, p1)                                      # a range: the same records
            assert np.array_equal(sub[0], rows[5:p1]) and np.array_equal(sub[1], scores[5:p1])
            st = bpr.resample(t, fm)
            assert (st["attempts"], st["forced"]) == (attempts, forced) and st == bpr.sample_stats
            if case == "forced":
                assert forced > 0 and (rows[ctx == 0] == 77).all()
            if n_cand == 1:
                assert st["replaced"] == 0
        close(bpr, fm)


# ---- 2. the scores --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [8, 64, 100, 200])
def test_scores_vs_fp64(fmhip, k):
    """Every candidate's device score yq_i + <q_u, q_i> against the fp64 score — topk_ref.pair_ref's S minus the per-context
    constant — within pair_ref's tolerance of the pair, the one test_gpu_topk.py applies to pairScores.  k = 8 (packed rows, 8
    lanes a pair), 64 (no packed slot, 16 lanes), 100 (32 lanes) and 200 (64 lanes: one pair a wave).  Item row 5 is empty: q = 0,
    its score is its prediction alone."""
    P = problem("base", k, seed=100 + k)
    bpr, fm = bref.build(fmhip, P, n_candidates=5)
    d = twin_draw(P, 3, 5)
    rows, scores = bpr.candidate_draws(fm, 3)
    assert np.array_equal(rows, d["rows"])
    err = np.abs(scores.astype(np.float64) - d["scores"])
    print("k = %d: max |device - fp64| / tol = %.3f" % (k, float((err / d["tol"]).max())))
    assert (err <= d["tol"]).all(), float((err / d["tol"]).max())
    assert (rows == 5).any()
    assert np.abs(d["scores"]).max() > 0.05                       # (the scores are not all about 0)
    close(bpr, fm)


# ---- 3. the choice, exact ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,batch_pairs", [(8, 0), (8, 128), (64, 0), (200, 128)])
def test_kept_row_is_the_first_strict_maximum_of_the_device_scores(fmhip, k, batch_pairs):
    """bpr.negatives() after resample(t, fm) against the first strict maximum of the scores the device itself recorded, for every
    pair, and `replaced` against the pairs whose kept candidate is not candidate 0."""
    P = problem("base", k, seed=200 + k)
    for n_cand in (2, 5, 64):
        bpr, fm = bref.build(fmhip, P, batch_pairs=batch_pairs, n_candidates=n_cand)
        for t in (0, 7):
            st = bpr.resample(t, fm)
            neg = bpr.negatives()
            rows, scores = bpr.candidate_draws(fm, t)
            keep = aref.first_strict_max(scores)
            assert np.array_equal(neg, rows[np.arange(len(neg)), keep])
            assert st["replaced"] == int((keep != 0).sum()) and 0 < st["replaced"] < len(neg)
            assert np.array_equal(bpr.negatives(), neg)                                   # the record mode left the mapping alone
        close(bpr, fm)


# ---- 4. the choice against fp64, with exact ties --------------------------------------------------------------------------------------------

def dyadic_problem(k=8, seed=7):
    """The dyadic-rational model of test_gpu_topk.py's exact case: V in multiples of 1/4 with |v| <= 1/2, w in multiples of 1/8,
    w0 = 1/4, x in {1, 1/2}, at most 3 entries a row.  40 contexts; 120 item rows drawn from 20 distinct ones, so different
    candidate rows tie exactly."""
    n1, n_ctx, M = 64, 40, 120
    rng = np.random.default_rng(seed)
    w0 = 0.25
    w = rng.integers(-4, 5, n1) / 8.0
    v = rng.integers(-2, 3, (k, n1)) / 4.0
    users = field_rows(seed + 1, n_ctx, [(0, 10), (10, 20), (20, 32)], empty=(4,), half=True)
    base = field_rows(seed + 2, 20, [(32, 40), (40, 52), (52, 64)], empty=(7,), half=True)
    pick = rng.integers(0, 20, M)
    lens = np.diff(base["row_ptr"])[pick]
    ptr = np.zeros(M + 1, np.int64)
    np.cumsum(lens, out=ptr[1:])
    sel = np.concatenate([np.arange(base["row_ptr"][p], base["row_ptr"][p + 1]) for p in pick])
    items = dict(row_ptr=ptr, col=base["col"][sel], val=base["val"][sel])
    flat = rng.choice(n_ctx * M, size=N_INTER, replace=False)
    positives = [np.sort(flat[flat // M == u] % M) for u in range(n_ctx)]
    ctx, cand, pptr, rows = bref.training_order(positives, M, seed, True)
    return dict(seed=seed, k=k, n1=n1, M=M, n_ctx=n_ctx, n_neg=1, shuffle=True, users=users, items=items, positives=positives, ctx=ctx,
                cand=cand, ptr=pptr, rows=rows, w0=w0, w=w, v=v)


def test_kept_rows_equal_the_twin_on_a_dyadic_model_with_ties(fmhip):
    """Every intermediate of s = yhat(i) + <q_u, q_i> is exact in fp32 on this model — checked here on the CPU by evaluating the
    expression in float32 and in float64 — so the device's scores equal the twin's exactly, duplicate item rows tie exactly, and the
    kept rows must be the twin's first strict maxima bit for bit."""
    P = dyadic_problem()
    T, _ = aref.score_table(P["w0"], P["w"], P["v"], P["users"], P["items"])
    from topk_ref import row_stats
    _, qc, _ = row_stats(P["w0"], P["w"], P["v"], P["users"])
    yd, qd, _ = row_stats(P["w0"], P["w"], P["v"], P["items"])
    dot32 = np.zeros(T.shape, np.float32)
    for f in range(P["k"]):
        dot32 += qc[:, f].astype(np.float32)[:, None] * qd[:, f].astype(np.float32)[None, :]
    T32 = yd.astype(np.float32)[None, :] + dot32
    assert T32.dtype == np.float32 and (T32.astype(np.float64) == T).all()
    # ... with room to spare: the scores are multiples of 2^-8 below 2^6
    assert (np.abs(T) < 64).all() and (T * 256 == np.round(T * 256)).all()
    for n_cand in (5, 64):
        bpr, fm = bref.build(fmhip, P, batch_pairs=128, n_candidates=n_cand)
        ties = 0
        for t in (0, 7):
            d = twin_draw(P, t, n_cand)
            rows, scores = bpr.candidate_draws(fm, t)
            assert np.array_equal(rows, d["rows"]) and np.array_equal(scores.astype(np.float64), d["scores"])
            st = bpr.resample(t, fm)
            assert np.array_equal(bpr.negatives(), d["neg"]) and st["replaced"] == d["replaced"]
            top = d["scores"] == d["scores"].max(axis=1, keepdims=True)
            ties += int(sum(len(set(r[m].tolist())) > 1 for r, m in zip(d["rows"], top)))
        assert ties > 10          # pairs whose best score is shared by different rows: the first one won
        close(bpr, fm)


# ---- 5. n_candidates = 1 is the uniform trainer ---------------------------------------------------------------------------------------------

def debug_inverse(bpr, batch, rows):
    from sparkfm_amd import _ffi
    cap = dict(trow=rows, tptr=rows + 1, tj=rows, wt=rows, wbeg=rows, wdst=rows, lt=rows // CUT + 1, lfirst=rows // CUT + 1, lcount=rows // CUT + 1,
               counts=4)
    out = {k: np.full(n, -7, np.int32) for k, n in cap.items()}
    _ffi.check(L().fmhip_bpr_debug_inverse(bpr.handle, batch, *[_ffi.ptr(out[k]) for k in cap]))
    return out


def check_inverse(bpr):
    """Every batch's device-built inverse map against append_batch of the batch's slice of the mapping as it stands (test_gpu_bpr.py's
    comparison)."""
    _, pos, neg = bpr.pairs()
    mi = np.empty(2 * len(neg), np.int32)
    mi[0::2], mi[1::2] = pos, neg
    for b in range(bpr.n_batches):
        r0, r1 = 2 * b * bpr.batch_pairs, min(len(mi), 2 * (b + 1) * bpr.batch_pairs)
        want = bref.append_batch(mi[r0:r1], CUT)
        got = debug_inverse(bpr, b, r1 - r0)
        nt, nw, nl, _ = want["counts"]
        assert got["counts"].tolist() == want["counts"].tolist(), (b, got["counts"], want["counts"])
        for key, n in (("trow", r1 - r0), ("tptr", nt + 1), ("tj", nt), ("wt", nw), ("wbeg", nw), ("wdst", nw), ("lt", nl), ("lfirst", nl), ("lcount", nl)):
            assert np.array_equal(got[key][:n], want[key]), (b, key)
            assert (got[key][n:] == -7).all(), (b, key)


def test_one_candidate_is_the_uniform_trainer(fmhip):
    """resample(t, fm) at n_candidates = 1 leaves the mapping, the inverse map and the attempts / forced of resample(t); two epochs
    with n_candidates=1 give the parameter bits, the AdaGrad state and last_stats of a handle built without the keyword."""
    P = bref.make_problem(300, 32, n_inter=N_INTER, n_neg=3)
    kw = dict(eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2], optimizer="adagrad")
    plain, fm0 = bref.build(fmhip, P, batch_pairs=700, **kw)
    one, fm1 = bref.build(fmhip, P, batch_pairs=700, n_candidates=1, **kw)
    for t in (0, 5):
        a, b = plain.resample(t), one.resample(t, fm1)
        assert b == dict(a, replaced=0) and np.array_equal(plain.negatives(), one.negatives())
        assert np.array_equal(one.negatives(), bref.draw(P, t)[0])
        for batch in range(one.n_batches):
            rows = 2 * min(700, one.n_pairs - 700 * batch)
            x, y = debug_inverse(plain, batch, rows), debug_inverse(one, batch, rows)
            assert all(np.array_equal(x[key], y[key]) for key in x)
        assert one.resample(t) == a                                 # without a model: still allowed at one candidate
    for _ in range(2):
        plain.learn(fm0)
        one.learn(fm1)
    assert same(params(fm0), params(fm1)) and same(get_state(fm0), get_state(fm1)) and plain.last_stats == one.last_stats
    assert np.array_equal(plain.negatives(), one.negatives()) and np.abs(fm1.v - P["v"]).max() > 1e-4
    close(plain, fm0)
    close(one, fm1)


# ---- 6. the epoch ---------------------------------------------------------------------------------------------------------------------------

def test_epoch_is_resample_plus_steps_and_reruns_are_bit_identical(fmhip):
    """learn at n_candidates = 4 against resample(t, fm) followed by step over the batches in order, bit for bit, for two epochs (the
    second one's candidates are scored by the model the first one trained); two fresh runs agree; the device-built inverse map after
    an adaptive resample is append_batch of the mapping."""
    P = bref.make_problem(310, 16, n_inter=N_INTER, n_neg=2)
    kw = dict(eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2], optimizer="adagrad", n_candidates=4)
    runs = []
    for _ in range(2):
        bpr, fm = bref.build(fmhip, P, batch_pairs=500, **kw)
        assert bpr.n_batches == 3
        for _ in range(2):
            bpr.learn(fm)
        runs.append((params(fm), bpr.negatives(), bpr.last_stats, get_state(fm)))
        close(bpr, fm)
    assert same(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2] and same(runs[0][3], runs[1][3])
    bpr, fm = bref.build(fmhip, P, batch_pairs=500, **kw)
    drawn = []
    for t in range(2):
        st = bpr.resample(t, fm)
        assert st["replaced"] > 0
        check_inverse(bpr)
        drawn.append(bpr.negatives())
        for b in range(bpr.n_batches):
            bpr.step(fm, b, want_stats=b == 0)
    assert same(params(fm), runs[0][0]) and same(get_state(fm), runs[0][3]) and np.array_equal(drawn[1], runs[0][1])
    # the draws were adaptive, and the second epoch's read the trained model
    assert not np.array_equal(drawn[0], bref.draw(P, 0)[0])
    assert not np.array_equal(drawn[1], twin_draw(P, 1, 4)["neg"])
    close(bpr, fm)


# ---- 7. harder on average -------------------------------------------------------------------------------------------------------------------

def test_adaptive_negatives_are_harder(fmhip):
    """After 10 epochs on bref.planted_task(3), the pairs drawn at n_candidates = 8 (t = 10) against the uniform draw of the same
    (seed, t) — candidate 0 of every pair — under the same model, margins yhat+ - yhat- in fp64: the kept candidate is the device's
    fp32 maximum over a set that holds candidate 0, so pair by pair its fp64 margin is at most the uniform one plus the two scores'
    tolerances (pair_ref's), and the mean is smaller."""
    T = bref.planted_task(3)
    P = aref.task_problem(T, 3, 8, 3)
    kw = dict(eta=1.0, reg0=0.0, regw=1e-3, regv=1e-3, optimizer="adagrad", adagrad_eps=EPS, adagrad_init=0.1)
    bpr, fm = bref.build(fmhip, P, batch_pairs=128, n_candidates=8, **kw)
    for _ in range(10):
        bpr.learn(fm)
    w0, w, v = params(fm)
    st = bpr.resample(10, fm)
    hard, uniform = bpr.negatives(), bref.draw(P, 10)[0]
    rows, _ = bpr.candidate_draws(fm, 10)
    assert np.array_equal(rows[:, 0], uniform) and (hard[:, None] == rows).any(axis=1).all()
    m_hard, m_uni = aref.margins(P, hard, w0, w, v), aref.margins(P, uniform, w0, w, v)
    _, tol = aref.score_table(w0, w, v, P["users"], P["items"])
    ctx = np.repeat(P["ctx"], P["n_neg"]).astype(np.int64)
    slack = tol[ctx, hard] + tol[ctx, uniform]
    print("mean margin: uniform %.4f, best of 8 %.4f; replaced %d of %d" % (m_uni.mean(), m_hard.mean(), st["replaced"], len(hard)))
    assert (m_hard <= m_uni + slack).all()
    assert m_hard.mean() < m_uni.mean() and st["replaced"] > len(hard) // 2
    close(bpr, fm)


# ---- 8. it learns -----------------------------------------------------------------------------------------------------------------------------

def run_task(fmhip, T, P, epochs, n_cand):
    kw = dict(eta=1.0, reg0=0.0, regw=1e-3, regv=1e-3, optimizer="adagrad", adagrad_eps=EPS, adagrad_init=0.1)
    bpr, fm = bref.build(fmhip, P, batch_pairs=128, n_candidates=n_cand, **kw)
    users, items = bpr.contexts, bpr.candidates
    untrained = fm.computeRankingMetrics(users, items, T["held_out"], k=10, exclude=T["train"])["ndcg"]
    pop = np.bincount(np.concatenate(T["train"]), minlength=P["M"]).astype(np.float64)
    popular = bref.ndcg_at(np.tile(pop, (P["n_ctx"], 1)), T["held_out"], T["train"])
    for _ in range(epochs):
        bpr.learn(fm)
    trained = fm.computeRankingMetrics(users, items, T["held_out"], k=10, exclude=T["train"])["ndcg"]
    ll = bpr.computePairLogLoss(fm)
    close(bpr, fm)
    return untrained, popular, trained, ll


def test_planted_preferences_are_learned_with_adaptive_negatives(fmhip):
    """bref.planted_task(3) exactly as test_gpu_bpr.py trains it (60 epochs of AdaGrad, eta 1.0, regw = regv = 1e-3, k = 8, n_neg = 3,
    batches of 128 pairs) at n_candidates = 8.  The fp64 twin's held-out NDCG@10 (computed on the CPU; test_host_bpr_adaptive.py
    pins it): untrained 0.0921, popularity 0.1994, uniform 0.6447, best of 8: 0.6308 — the task is too easy to need hard negatives,
    and the twin shows none gained.  Asserted: the model trained at n_candidates = 8 beats both baselines."""
    T = bref.planted_task(3)
    untrained, popular, trained, ll = run_task(fmhip, T, aref.task_problem(T, 3, 8, 3), 60, 8)
    print("planted, C = 8: ndcg@10 untrained %.4f popularity %.4f trained %.4f; pair log-loss of the last pairs %.4f" % (untrained, popular, trained, ll))
    assert popular == pytest.approx(0.1994, abs=5e-5)
    assert trained > popular and trained > untrained


def test_harder_planted_task_is_learned_with_adaptive_negatives(fmhip):
    """aref.hard_task(3): 60 users, 400 items under a popularity-skewed planted bias, 15 training and 5 held-out items a user; 30
    epochs (k = 8, n_neg = 3, batches of 128 pairs, the optimizer of the test above).  The fp64 twin's held-out NDCG@10 (CPU):
    untrained 0.0326, popularity 0.1193, uniform 0.1004 — below the popularity ranking — best of 8: 0.3064.  Asserted: the model
    trained at n_candidates = 8 beats both baselines."""
    T = aref.hard_task(3)
    untrained, popular, trained, ll = run_task(fmhip, T, aref.task_problem(T, 3, 8, 3), 30, 8)
    print("hard, C = 8: ndcg@10 untrained %.4f popularity %.4f trained %.4f; pair log-loss of the last pairs %.4f" % (untrained, popular, trained, ll))
    assert popular == pytest.approx(0.1193, abs=5e-5)
    assert trained > popular and trained > untrained


# ---- 9. refusals --------------------------------------------------------------------------------------------------------------------------------

def test_refusals(fmhip):
    from sparkfm_amd import _ffi
    P = problem("base")
    bpr, fm = bref.build(fmhip, P, batch_pairs=128, n_candidates=3)
    before = bpr.negatives()
    with pytest.raises(ValueError, match="needs a model"):
        bpr.resample(1)
    narrow = fmhip.FMModel(10, 8)
    with pytest.raises(_ffi.FmhipError, match="relational dataset has feature index .* num_attribute = 10") as ei:
        bpr.resample(1, narrow)
    assert ei.value.code == -4
    with pytest.raises(_ffi.FmhipError, match="num_attribute"):
        bpr.candidate_draws(narrow, 1)
    with pytest.raises(ValueError, match="non-empty range"):
        bpr.candidate_draws(fm, 1, 7, 7)
    with pytest.raises(ValueError, match="non-empty range"):
        bpr.candidate_draws(fm, 1, 0, bpr.n_pairs + 1)
    i, f = np.zeros(3, np.int32), np.zeros(3, np.float32)
    assert L().fmhip_bpr_debug_adaptive(fm.handle, bpr.handle, 1, 4, 4, _ffi.ptr(i), _ffi.ptr(f)) == -1 and b"pairs [4, 4)" in L().fmhip_last_error()
    assert L().fmhip_bpr_debug_adaptive(fm.handle, bpr.handle, 1, 0, 1, None, _ffi.ptr(f)) == -1 and b"NULL" in L().fmhip_last_error()
    assert L().fmhip_bpr_resample_adaptive(fm.handle, bpr.handle, -1, None) == -1 and b"t = -1" in L().fmhip_last_error()
    # the count: refused outside [1, 64] with a message that names it; the handle keeps what it had
    n = C.c_int32()
    for bad in (0, 65, -3):
        assert L().fmhip_bpr_set_candidates(bpr.handle, bad) == -1 and ("n_cand = %d" % bad).encode() in L().fmhip_last_error()
    assert L().fmhip_bpr_get_candidates(bpr.handle, C.byref(n)) == 0 and n.value == 3
    assert L().fmhip_bpr_get_candidates(bpr.handle, None) == -1 and b"n_cand is NULL" in L().fmhip_last_error()
    # nothing above moved the draw; fmhip_bpr_resample itself stays uniform whatever the count is
    assert np.array_equal(bpr.negatives(), before) and np.array_equal(before, bref.draw(P, 0)[0])
    st = _ffi.BprSampleStats()
    _ffi.check(L().fmhip_bpr_resample(bpr.handle, 4, C.byref(st)))
    assert np.array_equal(bpr.negatives(), bref.draw(P, 4)[0])
    # ... and the handle still resamples adaptively (stats nullable)
    _ffi.check(L().fmhip_bpr_resample_adaptive(fm.handle, bpr.handle, 4, None))
    rows, scores = bpr.candidate_draws(fm, 4)
    assert np.array_equal(bpr.negatives(), rows[np.arange(len(rows)), aref.first_strict_max(scores)])
    assert not np.array_equal(bpr.negatives(), bref.draw(P, 4)[0])
    narrow.close()
    close(bpr, fm)


# ---- 10. include/sparkfm.hpp ------------------------------------------------------------------------------------------------------------------------

def test_cpp_bpr_adaptive_matches_python(fmhip, tmp_path):
    """tests/cpp_bpr_adaptive.cpp (include/sparkfm.hpp's HipBPR with n_candidates = 4) against the Python mirror over the integer
    formulas of tests/cpp_bpr.cpp: the draw after two epochs, the statistics and the draw of an adaptive resample at t = 2, and every
    parameter, hex floats equal."""
    from sparkfm_amd import _build
    from test_gpu_bpr import cpp_problem
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_bpr_adaptive")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_bpr_adaptive.cpp"), "-L" + _build.LIBDIR, "-lfmhip",
                           "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = {ln.split()[0]: [float.fromhex(t) for t in ln.split()[1:]] for ln in out.stdout.decode().splitlines()}
    c = cpp_problem()
    mk = lambda b: fmhip.DataSet(b["row_ptr"], b["col"], b["val"], np.zeros(len(b["row_ptr"]) - 1), batch_rows=0)      # noqa: E731
    bpr = fmhip.HipBPR.run(mk(c["users"]), mk(c["items"]), c["positives"], n_neg=2, batch_pairs=100, seed=5, shuffle=False, eta=0.05, regw=1e-4,
                           regv=1e-4, n_candidates=4)
    fm = fmhip.FMModel(c["n1"] - 1, c["k"])
    fm.w0, fm.w, fm.v = c["w0"], c["w"], c["v"]
    bpr.learn(fm)
    bpr.learn(fm)
    assert got["candidates"] == [4] and got["neg"] == bpr.negatives().tolist()
    st = bpr.resample(2, fm)
    assert got["attempts"] == [st["attempts"]] and got["forced"] == [st["forced"]] and got["replaced"] == [st["replaced"]] and st["replaced"] > 0
    assert got["neg2"] == bpr.negatives().tolist()
    assert got["w0"] == [fm.w0] and got["w"] == fm.w.tolist() and got["v"] == fm.v.reshape(-1, order="F").tolist()
    close(bpr, fm)
