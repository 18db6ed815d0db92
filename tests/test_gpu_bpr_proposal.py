"""The BPR trainer's weighted proposal on the GPU (include/fmhip_proposal.h) against the fp64 twin of bpr_proposal_ref.py: the
keep-the-draw rule's rows and counters bit for bit, the table, the forced walk, every candidate row of the two record calls at the
narrowest and the widest lane group, the scored rules' choice on the device's own scores, the reset to the uniform proposal, the
per-batch redraw's invariant, a trajectory, and the harder planted task.

The base shape is bpr_ref.make_problem's 40 contexts x 120 items with 600 interactions."""
import numpy as np
import pytest

import bpr_adaptive_ref as aref
import bpr_proposal_ref as pref
import bpr_ref as bref
import train_ref as ref
import warp_ref as wref
from test_gpu_adagrad import EPS, get_state
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


def params(fm):
    return fm.w0, fm.w.copy(), fm.v.copy()


def close(bpr, fm=None):
    bpr.close()
    bpr.contexts.unpersist()
    bpr.candidates.unpersist()
    if fm is not None:
        fm.close()


def given_weights(M, seed=7):
    """An explicit weight vector: log-normal, so a few rows carry most of the mass and most buckets are redirected."""
    return np.exp(np.random.default_rng(seed).normal(0.0, 1.5, M))


def forced_problem(seed, k=8, n_ctx=40, M=120, n_inter=600):
    """The base shape with context 0 holding 119 of the 120 rows (all but row 77)."""
    rng = np.random.default_rng(seed)
    flat = rng.choice((n_ctx - 1) * M, size=n_inter - (M - 1), replace=False)
    positives = [np.setdiff1d(np.arange(M), [77])] + [np.sort(flat[flat // M == u] % M) for u in range(n_ctx - 1)]
    return bref.make_problem(seed, k, n_inter=n_inter, positives=positives)


def pair_ctx(P):
    return np.repeat(P["ctx"], P["n_neg"]).astype(np.int64)


# ---- 1. keep the draw ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("how", ["popularity", "given"])
def test_keep_the_draw_equals_the_twin(fmhip, how):
    """n_candidates = 1 under negatives="popularity" and under an explicit weight vector, at t = 0 and t = 7: negatives() against
    the twin bit for bit, sample_stats against the twin's attempts and forced counts; n_neg = 2 and three batches, the last short."""
    P = bref.make_problem(500, 8, n_neg=2)
    w = pref.popularity(P) if how == "popularity" else given_weights(P["M"])
    bpr, fm = bref.build(fmhip, P, batch_pairs=500, negatives="popularity" if how == "popularity" else w)
    assert np.array_equal(bpr.proposal, w) and bpr.n_batches == 3
    table = pref.alias_table(w)
    assert np.array_equal(bpr.negatives(), bref.draw(P, 0)[0])      # a fresh handle holds the uniform draw at t = 0
    for t in (0, 7):
        want, attempts, forced = pref.draw(P, t, table)
        st = bpr.resample(t)
        got = bpr.negatives()
        assert got.dtype == np.int32 and np.array_equal(got, want)
        assert st == dict(attempts=attempts, forced=forced) == bpr.sample_stats
        assert not np.array_equal(got, bref.draw(P, t)[0])
    close(bpr, fm)


# ---- 2. the table and the forced walk -----------------------------------------------------------------------------------------------------

def test_table_and_forced_walk(fmhip):
    """proposal_table() against the twin's table entry for entry; context 0 holds 119 of the 120 rows: every one of its pairs gets
    row 77, most of them by the forced walk, and the counters are the twin's."""
    P = forced_problem(501)
    w = given_weights(P["M"], 8)
    bpr, fm = bref.build(fmhip, P, batch_pairs=128, negatives=w)
    thresh, alias = bpr.proposal_table()
    want = pref.alias_table(w)
    assert thresh.dtype == np.uint32 and alias.dtype == np.int32
    assert np.array_equal(thresh, want[0]) and np.array_equal(alias, want[1]) and (alias != np.arange(P["M"])).sum() > 60
    ctx = pair_ctx(P)
    for t in (0, 7):
        neg, attempts, forced = pref.draw(P, t, want)
        st = bpr.resample(t)
        assert np.array_equal(bpr.negatives(), neg) and st == dict(attempts=attempts, forced=forced)
        assert forced > 0 and (neg[ctx == 0] == 77).all() and (ctx == 0).sum() == 119
    close(bpr, fm)


# ---- 3. the record calls ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [8, 200])
@pytest.mark.parametrize("sampler", ["auto", "warp"])
def test_record_calls_give_the_twins_candidates(fmhip, k, sampler):
    """candidate_draws(fm, t) at n_candidates = 8 and warp_draws(fm, t): every candidate ROW against the twin's candidate c, candidate
    0 against the n_candidates = 1 draw, at k = 8 (Kp = 32: lane groups of 8, the narrowest walk) and k = 200 (Kp = 256: groups of
    64, the widest); the scores against the fp64 score table within topk_ref.pair_ref's tolerance of the pair, as
    test_gpu_bpr_adaptive.py and test_gpu_warp.py check theirs.  Context 0 has one row left: its candidates are all row 77."""
    P = forced_problem(510 + k, k)
    w = pref.popularity(P)
    table = pref.alias_table(w)
    ctx, pos = pair_ctx(P), np.repeat(P["cand"], P["n_neg"]).astype(np.int64)
    bpr, fm = bref.build(fmhip, P, batch_pairs=128, n_candidates=8, sampler=sampler, negatives="popularity")
    T, tol = aref.score_table(P["w0"], P["w"], P["v"], P["users"], P["items"])
    for t in (0, 7):
        want, _, _ = pref.candidates(P["seed"], t, ctx, P["ptr"], P["rows"], P["M"], 8, table)
        if sampler == "warp":
            rows, scores, pos_scores = bpr.warp_draws(fm, t)
            perr = np.abs(pos_scores.astype(np.float64) - T[ctx, pos])
            assert (perr <= tol[ctx, pos]).all(), float((perr / tol[ctx, pos]).max())
        else:
            rows, scores = bpr.candidate_draws(fm, t)
        assert rows.dtype == np.int32 and rows.shape == (len(ctx), 8) and np.array_equal(rows, want)
        assert np.array_equal(rows[:, 0], pref.draw(P, t, table)[0])
        assert (rows[ctx == 0] == 77).all() and (rows[ctx != 0, 1] != rows[ctx != 0, 0]).mean() > 0.8
        err = np.abs(scores.astype(np.float64) - T[ctx[:, None], rows])
        print("k = %d, %s, t = %d: max |device - fp64| / tol = %.3f" % (k, sampler, t, float((err / tol[ctx[:, None], rows]).max())))
        assert scores.dtype == np.float32 and (err <= tol[ctx[:, None], rows]).all()
        sub = bpr.warp_draws(fm, t, 5, 38) if sampler == "warp" else bpr.candidate_draws(fm, t, 5, 38)
        assert np.array_equal(sub[0], rows[5:38]) and np.array_equal(sub[1], scores[5:38])
    close(bpr, fm)


@pytest.mark.parametrize("k", [8, 200])
def test_scored_rules_choose_among_the_proposals_candidates(fmhip, k):
    """resample(t, fm) under the weighted proposal: the best-of-5 rule keeps the first strict maximum of the scores the device itself
    recorded, with the twin's attempts and forced counts; WARP at 8 candidates keeps the first violator of them, with the weights of
    the unchanged table W[N] = H((M - 1) // N)."""
    P = bref.make_problem(520 + k, k)
    w = given_weights(P["M"], 9)
    table = pref.alias_table(w)
    ctx = pair_ctx(P)
    bpr, fm = bref.build(fmhip, P, batch_pairs=128, n_candidates=5, negatives=w)
    for t in (0, 7):
        st = bpr.resample(t, fm)
        rows, scores = bpr.candidate_draws(fm, t)
        want, attempts, forced = pref.candidates(P["seed"], t, ctx, P["ptr"], P["rows"], P["M"], 5, table)
        keep = aref.first_strict_max(scores)
        assert np.array_equal(rows, want) and np.array_equal(bpr.negatives(), rows[np.arange(len(ctx)), keep])
        assert st == dict(attempts=attempts, forced=forced, replaced=int((keep != 0).sum())) and 0 < st["replaced"] < len(ctx)
    close(bpr, fm)
    bpr, fm = bref.build(fmhip, P, batch_pairs=128, n_candidates=8, sampler="warp", margin=0.05, negatives=w)
    for t in (0, 7):
        st = bpr.resample(t, fm)
        rows, scores, pos = bpr.warp_draws(fm, t)
        n_first = wref.first_violator(scores, pos, 0.05)
        neg, cw = wref.choose(rows, n_first, wref.weight_table(P["M"], 8))
        assert np.array_equal(bpr.negatives(), neg) and np.array_equal(bpr.trials(), n_first) and np.array_equal(bpr.pair_weights(), cw)
        assert st == dict(pairs=len(ctx), violated=int((n_first > 0).sum()), trials=int(n_first.sum())) and 0 < st["violated"] < len(ctx)
    close(bpr, fm)


# ---- 4. the reset ----------------------------------------------------------------------------------------------------------------------------

def test_reset_gives_the_uniform_bits(fmhip):
    """After set_proposal(None) negatives() at a given (seed, t) is that of a handle whose proposal was never set; a handle made
    with negatives="uniform" matches bpr_ref.sample as it always did; a refused vector leaves the proposal in force; and the
    proposal moves with set_proposal from the next draw on, the standing draw left as it is."""
    import ctypes as C
    from sparkfm_amd import _ffi
    P = bref.make_problem(530, 8)
    w = pref.popularity(P)
    plain, fm0 = bref.build(fmhip, P, batch_pairs=128)
    uniform, fm1 = bref.build(fmhip, P, batch_pairs=128, negatives="uniform")
    bpr, fm = bref.build(fmhip, P, batch_pairs=128, negatives="popularity")
    flag = C.c_int(-1)
    L = _ffi.load()
    assert L.fmhip_proposal_get(plain.handle, C.byref(flag)) == 0 and flag.value == 0
    assert L.fmhip_proposal_get(bpr.handle, C.byref(flag)) == 0 and flag.value == 1
    assert L.fmhip_proposal_table(plain.handle, None, None) == -1 and b"the proposal is uniform" in L.fmhip_last_error()
    bpr.resample(3)
    weighted = bpr.negatives()
    assert np.array_equal(weighted, pref.draw(P, 3, pref.alias_table(w))[0])
    # the C call's refusals: the first bad row named, the proposal and the standing draw left alone
    for at, bad in ((5, 0.0), (0, -1.0), (119, np.nan), (17, np.inf)):
        wb = w.copy()
        wb[at] = bad
        wb[119] = bad if at == 119 else -3.0
        assert L.fmhip_proposal_set(bpr.handle, _ffi.ptr(wb)) == -1 and ("weights[%d]" % at).encode() in L.fmhip_last_error()
        with pytest.raises(ValueError, match=r"weights\[%d\]" % at):
            bpr.set_proposal(wb)
    assert np.array_equal(bpr.proposal, w) and np.array_equal(bpr.proposal_table()[0], pref.alias_table(w)[0])
    assert np.array_equal(bpr.negatives(), weighted)
    bpr.resample(3)
    assert np.array_equal(bpr.negatives(), weighted)
    # the reset
    bpr.set_proposal(None)
    assert bpr.proposal is None and np.array_equal(bpr.negatives(), weighted)      # (takes effect with the next draw)
    assert L.fmhip_proposal_get(bpr.handle, C.byref(flag)) == 0 and flag.value == 0
    for t in (3, 0):
        sts = [b.resample(t) for b in (bpr, plain, uniform)]
        want, attempts, forced = bref.draw(P, t)
        assert sts[0] == sts[1] == sts[2] == dict(attempts=attempts, forced=forced)
        assert np.array_equal(bpr.negatives(), want) and np.array_equal(plain.negatives(), want) and np.array_equal(uniform.negatives(), want)
    # ... and back, on a handle that never had one
    w2 = given_weights(P["M"], 11)
    plain.set_proposal(w2)
    plain.resample(5)
    assert np.array_equal(plain.negatives(), pref.draw(P, 5, pref.alias_table(w2))[0])
    for b, m in ((plain, fm0), (uniform, fm1), (bpr, fm)):
        close(b, m)


# ---- 5. the redraw -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
def test_per_batch_redraw_trains_the_per_epoch_bits(fmhip, optimizer):
    """redraw="batch" under the keep-the-draw rule and negatives="popularity", three batches of 151 pairs and a last one of 146, one
    epoch: the parameters' bytes, the optimizer's state and negatives() are those of redraw="epoch" — the draw reads no model,
    whatever the proposal — and negatives() is the twin's draw."""
    P = bref.make_problem(540, 8, n_neg=1, n_inter=599)
    kw = dict(optimizer=optimizer, eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2])
    if optimizer == "adagrad":
        kw.update(adagrad_eps=EPS, adagrad_init=0.1)
    out = []
    for redraw in ("epoch", "batch"):
        bpr, fm = bref.build(fmhip, P, batch_pairs=151, redraw=redraw, negatives="popularity", **kw)
        assert bpr.n_batches == 4 and 599 - 3 * 151 == 146
        bpr._epoch = 2
        bpr.learn(fm)
        out.append((params(fm), get_state(fm) if optimizer == "adagrad" else (), bpr.negatives(), bpr.sample_stats if redraw == "batch" else None))
        close(bpr, fm)
    a, b = out
    assert same(a[0], b[0]) and same(a[1], b[1]) and np.array_equal(a[2], b[2])
    want, attempts, forced = pref.draw(P, 2, pref.alias_table(pref.popularity(P)))
    assert np.array_equal(b[2], want) and np.abs(b[0][2] - P["v"]).max() > 1e-4
    assert (b[3]["pairs"], b[3]["attempts"], b[3]["forced"]) == (599, attempts, forced)


# ---- 6. a trajectory -------------------------------------------------------------------------------------------------------------------------------

def test_five_epochs_vs_twin(fmhip):
    """Five epochs of HipBPR.learn under negatives="popularity", two batches, n_neg = 3 (1800 pairs), against the fp64 twin — the
    bpr_ref.epochs step with the twin's weighted draws: rel-L2 1e-5 on v and w, test_gpu_bpr.py's bound for the same comparison.
    The draws read no model, so both sides train on identical pairs."""
    P = bref.make_problem(550, 16, n_neg=3)
    bpr, fm = bref.build(fmhip, P, batch_pairs=900, eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2], negatives="popularity")
    for _ in range(5):
        bpr.learn(fm)
    assert bpr.last_stats["rows"] == 3600 and bpr.last_stats["steps"] == 2 and bpr.last_stats["sum_e"] == 0.0
    table = pref.alias_table(pref.popularity(P))
    s, got = pref.epochs(ref.State(P["w0"], P["w"], P["v"]), P, 5, 900, ETA, *REGS, ref.Rule("logistic", True, None), table)
    assert np.array_equal(bpr.negatives(), got["neg"]) and np.array_equal(got["neg"], pref.draw(P, 4, table)[0])
    assert rel(fm.v, s.v) <= 1e-5 and rel(fm.w, s.w) <= 1e-5, (rel(fm.v, s.v), rel(fm.w, s.w))
    assert fm.w0 == pytest.approx(s.w0, rel=1e-5, abs=1e-6)
    assert np.abs(fm.v - P["v"]).max() > 1e-4
    close(bpr, fm)


# ---- 7. it learns ------------------------------------------------------------------------------------------------------------------------------------

def test_harder_planted_task_under_the_popularity_proposal(fmhip):
    """aref.hard_task(3) as test_gpu_bpr_adaptive.py trains it (30 epochs, k = 8, n_neg = 3, batches of 128 pairs, AdaGrad eta 1.0,
    regw = regv = 1e-3) at n_candidates = 1 under negatives="popularity".  The fp64 twin's held-out NDCG@10 (CPU;
    test_host_bpr_proposal.py pins it): 0.1693, against 0.1004 for the uniform proposal and 0.1193 for the popularity ranking.
    Asserted, as there: the trained model beats the popularity ranking and the untrained model."""
    T = aref.hard_task(3)
    P = aref.task_problem(T, 3, 8, 3)
    kw = dict(eta=1.0, reg0=0.0, regw=1e-3, regv=1e-3, optimizer="adagrad", adagrad_eps=EPS, adagrad_init=0.1)
    bpr, fm = bref.build(fmhip, P, batch_pairs=128, negatives="popularity", **kw)
    users, items = bpr.contexts, bpr.candidates
    untrained = fm.computeRankingMetrics(users, items, T["held_out"], k=10, exclude=T["train"])["ndcg"]
    pop = np.bincount(np.concatenate(T["train"]), minlength=P["M"]).astype(np.float64)
    popular = bref.ndcg_at(np.tile(pop, (P["n_ctx"], 1)), T["held_out"], T["train"])
    for _ in range(30):
        bpr.learn(fm)
    trained = fm.computeRankingMetrics(users, items, T["held_out"], k=10, exclude=T["train"])["ndcg"]
    print("hard, popularity^0.75, C = 1: ndcg@10 untrained %.4f popularity ranking %.4f trained %.4f (twin 0.1693)" % (untrained, popular, trained))
    assert popular == pytest.approx(0.1193, abs=5e-5)
    assert trained > popular and trained > untrained
    close(bpr, fm)


# ---- 8. include/sparkfm.hpp ------------------------------------------------------------------------------------------------------------------------

def test_cpp_proposal_matches_python(fmhip, tmp_path):
    """tests/cpp_bpr_proposal.cpp (include/sparkfm.hpp's HipBPR with negatives = kPopularity) against the Python mirror over the
    integer formulas of tests/cpp_bpr.cpp: the popularity weights (to one ulp: pow is the platform's on either side), and with the
    C++ side's weights handed to the mirror the table, the draw at t = 2 and its counters, the draw and every parameter after one
    epoch, and the uniform draw after the reset, hex floats equal."""
    import os
    import subprocess
    from sparkfm_amd import _build
    from test_gpu_bpr import cpp_problem
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_bpr_proposal")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_bpr_proposal.cpp"), "-L" + _build.LIBDIR, "-lfmhip",
                           "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = {ln.split()[0]: [float.fromhex(t) for t in ln.split()[1:]] for ln in out.stdout.decode().splitlines()}
    c = cpp_problem()
    mk = lambda b: fmhip.DataSet(b["row_ptr"], b["col"], b["val"], np.zeros(len(b["row_ptr"]) - 1), batch_rows=0)      # noqa: E731
    kw = dict(n_neg=2, batch_pairs=100, seed=5, shuffle=False, eta=0.05, regw=1e-4, regv=1e-4)
    named = fmhip.HipBPR.run(mk(c["users"]), mk(c["items"]), c["positives"], negatives="popularity", **kw)
    w = np.array(got["weights"])
    assert np.allclose(named.proposal, w, rtol=4e-16, atol=0) and len(set(got["weights"])) > 3
    bpr = fmhip.HipBPR.run(named.contexts, named.candidates, c["positives"], negatives=w, **kw)
    fm = fmhip.FMModel(c["n1"] - 1, c["k"])
    fm.w0, fm.w, fm.v = c["w0"], c["w"], c["v"]
    thresh, alias = bpr.proposal_table()
    assert got["thresh"] == thresh.tolist() and got["alias"] == alias.tolist()
    assert np.array_equal(thresh, pref.alias_table(w)[0]) and np.array_equal(alias, pref.alias_table(w)[1])
    st = bpr.resample(2)
    assert got["neg"] == bpr.negatives().tolist() and got["stats"] == [st["attempts"], st["forced"]]
    bpr.learn(fm)
    assert got["neg1"] == bpr.negatives().tolist()
    assert got["w0"] == [fm.w0] and got["w"] == fm.w.tolist() and got["v"] == fm.v.T.ravel().tolist()
    bpr.set_proposal(None)
    bpr.resample(2)
    assert got["neg_uniform"] == bpr.negatives().tolist() and got["neg_uniform"] != got["neg"]
    close(bpr, fm)
