"""The BPR trainer on the GPU (include/fmhip_bpr.h) against the fp64 twin of bpr_ref.py: the device sampler's draws bit for bit, the
device-built inverse map of the candidates relation against the Python append_batch, one step against the twin and against the
flat pair step on expand(), a three-epoch trajectory, bit-identical reruns, the create refusals, a planted preference task, and
include/sparkfm.hpp's HipBPR."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bpr_ref as bref
import relational_ref as rref
import train_ref as ref
from test_gpu_adagrad import EPS, check_step as check_adagrad_step, get_state
from test_gpu_weights import check_step
from train_ref import rel, same

pytestmark = pytest.mark.gpu

REGS = (1e-3, 2e-3, 3e-3)
ETA = 0.05
CUT = 256


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


def forced_positives(seed, n_ctx=40, M=120, n_inter=600):
    """The base problem's shape with context 0 holding 119 of the 120 rows (all but row 77)."""
    rng = np.random.default_rng(seed)
    flat = rng.choice((n_ctx - 1) * M, size=n_inter - (M - 1), replace=False)
    return [np.setdiff1d(np.arange(M), [77])] + [np.sort(flat[flat // M == u] % M) for u in range(n_ctx - 1)]


# ---- 1. the draws -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["base_1", "base_3", "forced", "two_candidates"])
def test_draws_equal_the_twin(fmhip, case):
    """bpr.negatives() after resample(t), t in {0, 1, 7}, and sample_stats against the twin, bit for bit — on the base problem (n_neg
    1 and 3), with a context that holds 119 of 120 rows (its pairs get row 77; most are forced), and on a 2-candidate block."""
    if case == "forced":
        P = bref.make_problem(31, 8, n_neg=2, positives=forced_positives(31))
    elif case == "two_candidates":
        P = bref.make_problem(32, 8, n_ctx=9, M=2, n_neg=3, positives=[[u % 2] if u % 3 else [] for u in range(9)])
    else:
        P = bref.make_problem(30, 8, n_neg=int(case[-1]))
    bpr, fm = bref.build(fmhip, P, batch_pairs=128)
    ctx = np.repeat(P["ctx"], P["n_neg"])
    assert np.array_equal(bpr.inter_ctx, P["ctx"]) and np.array_equal(bpr.inter_cand, P["cand"])
    assert np.array_equal(bpr.negatives(), bref.draw(P, 0)[0])                # create draws at t = 0
    for t in (0, 1, 7):
        neg, attempts, forced = bref.draw(P, t)
        st = bpr.resample(t)
        got = bpr.negatives()
        assert got.dtype == np.int32 and np.array_equal(got, neg)
        assert st == dict(attempts=attempts, forced=forced) == bpr.sample_stats
        c, pos, n = bpr.pairs()
        assert np.array_equal(c, ctx) and np.array_equal(pos, np.repeat(P["cand"], P["n_neg"])) and np.array_equal(n, neg)
    if case == "forced":
        assert forced > 0 and (neg[ctx == 0] == 77).all()
    info = bpr.info()
    assert info == dict(n_pairs=len(ctx), dimension=bpr.dimension, batch_pairs=min(128, len(ctx)), n_batches=-(-len(ctx) // 128), n_neg=P["n_neg"])
    close(bpr, fm)


# ---- 2. the device inverse map ---------------------------------------------------------------------------------------------------------

def debug_inverse(bpr, batch, rows):
    from sparkfm_amd import _ffi
    cap = dict(trow=rows, tptr=rows + 1, tj=rows, wt=rows, wbeg=rows, wdst=rows, lt=rows // CUT + 1, lfirst=rows // CUT + 1, lcount=rows // CUT + 1,
               counts=4)
    out = {k: np.full(n, -7, np.int32) for k, n in cap.items()}
    _ffi.check(L().fmhip_bpr_debug_inverse(bpr.handle, batch, *[_ffi.ptr(out[k]) for k in cap]))
    return out


def check_inverse(bpr, t):
    """Every batch's device-built inverse map against append_batch of the batch's slice of the sampled mapping."""
    bpr.resample(t)
    ctx, pos, neg = bpr.pairs()
    mi = np.empty(2 * len(neg), np.int32)
    mi[0::2], mi[1::2] = pos, neg
    seen = dict(long=0, partial=0, max_len=0, touched=0)
    for b in range(bpr.n_batches):
        r0, r1 = 2 * b * bpr.batch_pairs, min(len(mi), 2 * (b + 1) * bpr.batch_pairs)
        want = bref.append_batch(mi[r0:r1], CUT)
        got = debug_inverse(bpr, b, r1 - r0)
        nt, nw, nl, _ = want["counts"]
        assert got["counts"].tolist() == want["counts"].tolist(), (b, got["counts"], want["counts"])
        for key, n in (("trow", r1 - r0), ("tptr", nt + 1), ("tj", nt), ("wt", nw), ("wbeg", nw), ("wdst", nw), ("lt", nl), ("lfirst", nl), ("lcount", nl)):
            assert np.array_equal(got[key][:n], want[key]), (b, key)
            assert (got[key][n:] == -7).all(), (b, key)           # nothing written past the entries that count
        lens = np.diff(want["tptr"])
        seen["long"] += nl
        seen["partial"] += int((lens[lens > CUT] % CUT != 0).sum())
        seen["max_len"] = max(seen["max_len"], int(lens.max()))
        seen["touched"] = max(seen["touched"], int(nt))
        seen.setdefault("lens", []).extend(lens.tolist())
    return seen


@pytest.mark.parametrize("n_neg,batch_pairs", [(1, 0), (3, 128), (3, 0)])
def test_device_inverse_map_on_the_base_problem(fmhip, n_neg, batch_pairs):
    P = bref.make_problem(40 + n_neg, 8, n_neg=n_neg)
    bpr, fm = bref.build(fmhip, P, batch_pairs=batch_pairs)
    for t in (0, 3):
        seen = check_inverse(bpr, t)
        assert seen["touched"] > 60
    close(bpr, fm)


def test_device_inverse_map_with_long_lists(fmhip):
    """A 3-candidate block, 1000 pairs in training order by context (no shuffle), batches of 512 pairs.  Contexts 0 .. 254 hold rows
    {0, 1} (their negative is row 2, whatever is drawn), context 255 holds {0, 2} (negative: row 1): batch 0 is their 512 pairs, and its
    lists hold exactly 256 (row 0: one whole item at the cut), 257 (row 1: the shortest long list, a partial chunk of one row) and 511
    rows.  Contexts 256 .. 743 hold one row each: batch 1's 488 pairs draw freely, lists of several hundred rows."""
    positives = [[0, 1]] * 255 + [[0, 2]] + [[u % 3] for u in range(488)]
    P = bref.make_problem(50, 8, n_ctx=744, M=3, n_neg=1, shuffle=False, positives=positives)
    bpr, fm = bref.build(fmhip, P, batch_pairs=512)
    assert bpr.n_pairs == 1000 and bpr.n_batches == 2
    seen = check_inverse(bpr, 0)
    assert seen["lens"][:3] == [256, 257, 511] and seen["long"] >= 4 and seen["partial"] >= 3 and min(seen["lens"][3:]) > 200
    check_inverse(bpr, 9)
    # ... and the step runs on them: one epoch against the twin
    s, _ = bref.epochs(ref.State(P["w0"], P["w"], P["v"]), P, 1, 512, ETA, *REGS, ref.Rule("logistic", True, None), t0=4)
    bpr.eta, (bpr.reg0, bpr.regw, bpr.regv) = ETA, REGS
    bpr._epoch = 4
    bpr.learn(fm)
    assert rel(fm.v, s.v) <= 1e-5 and rel(fm.w, s.w) <= 1e-5, (rel(fm.v, s.v), rel(fm.w, s.w))
    close(bpr, fm)


def test_device_inverse_map_when_most_rows_are_untouched(fmhip):
    """5000 candidate rows, 150 pairs per batch: a batch touches at most 300 of them."""
    rng = np.random.default_rng(60)
    flat = rng.choice(40 * 5000, size=300, replace=False)
    positives = [np.sort(flat[flat // 5000 == u] % 5000) for u in range(40)]
    P = bref.make_problem(60, 8, M=5000, n_neg=1, positives=positives, item_ids=(100, 400))
    bpr, fm = bref.build(fmhip, P, batch_pairs=150)
    seen = check_inverse(bpr, 2)
    assert 250 < seen["touched"] <= 300 and seen["long"] == 0
    close(bpr, fm)


# ---- 3. one step against the twin and against the flat route -----------------------------------------------------------------------------

# k -> Kp: 8 -> 32 (packed e), 64 -> 64 (e embedded in the row's low bits), 200 -> 256 (packed)
@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
@pytest.mark.parametrize("loss", ["logistic", "squared"])
@pytest.mark.parametrize("k", [8, 64, 200])
def test_one_step_vs_twin_and_flat(fmhip, k, loss, optimizer):
    """fmhip_bpr_step on batch 1 of 2 of the base problem (n_neg = 1, 300 pairs a batch) against the twin — check_step of
    test_gpu_weights.py / test_gpu_adagrad.py, the project's tolerances — and, by the same check, against HipSGD(pairs=True).step on
    bpr.expand() from the same initial model.  Statistics: rows = 2 * pairs, sum_e exactly 0, sse = 2 sum g^2 to rel 1e-5."""
    P = bref.make_problem(100 + k, k, n_neg=1)
    kw = dict(loss=loss, optimizer=optimizer, eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2])
    if optimizer == "adagrad":
        kw.update(adagrad_eps=EPS, adagrad_init=0.1)
    bpr, fm = bref.build(fmhip, P, batch_pairs=300, **kw)
    bpr.resample(2)
    p = bref.layout(P, bref.draw(P, 2)[0])
    init = 0.1 if optimizer == "adagrad" else 0.0
    s0 = ref.State(P["w0"], P["w"], P["v"], init)
    rule = ref.Rule(loss, True, EPS if optimizer == "adagrad" else None)
    s1 = bref.step(s0.copy(), p, 600, 1200, ETA, *REGS, rule)
    e = bref.gradient(s0, p, 600, 1200, loss)[2]
    st = bpr.step(fm, 1)
    check = (lambda m, a, b: check_adagrad_step(m, a, b, 0.1, ETA)) if optimizer == "adagrad" else check_step
    check(fm, s0, s1)
    assert st["rows"] == 600 and st["steps"] == 1 and st["nonfinite"] == 0 and st["sum_e"] == 0.0
    assert st["sse"] == pytest.approx((e * e).sum(), rel=1e-5)
    # the flat route: the same pairs, joined, through the flat pair step
    fl = bpr.expand().cache()
    assert fl.size == 1200 and fl.n_batches == 2
    fm2 = fmhip.FMModel(P["n1"] - 1, k)
    fm2.w0, fm2.w, fm2.v = P["w0"], P["w"], P["v"]
    st2 = fmhip.HipSGD(pairs=True, **kw).step(fm2, fl, 1)
    f1 = ref.State(fm2.w0, fm2.w, fm2.v)
    if optimizer == "adagrad":
        f1.n0, f1.nw, f1.nv = get_state(fm2)
    check(fm, s0, f1)
    assert st2["rows"] == 600 and st2["sum_e"] == 0.0 and st["sse"] == pytest.approx(st2["sse"], rel=1e-5)
    fl.unpersist()
    fm2.close()
    close(bpr, fm)


# ---- 4. a trajectory ------------------------------------------------------------------------------------------------------------------------

def test_three_epochs_vs_twin(fmhip):
    """Three epochs of two batches, n_neg = 3 (1800 pairs): rel-L2 1e-5 on v and w against the twin — the relational tests' bound.  The
    draws do not depend on the model, so both sides train on identical pairs; the pair log-loss of the last draw to rel 1e-5."""
    P = bref.make_problem(200, 16, n_neg=3)
    bpr, fm = bref.build(fmhip, P, batch_pairs=900, eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2])
    assert bpr.n_batches == 2
    for _ in range(3):
        bpr.learn(fm)
    assert bpr.last_stats["rows"] == 3600 and bpr.last_stats["steps"] == 2 and bpr.last_stats["sum_e"] == 0.0
    s, p = bref.epochs(ref.State(P["w0"], P["w"], P["v"]), P, 3, 900, ETA, *REGS, ref.Rule("logistic", True, None))
    assert np.array_equal(bpr.negatives(), p["maps"][1][1::2])
    assert rel(fm.v, s.v) <= 1e-5 and rel(fm.w, s.w) <= 1e-5, (rel(fm.v, s.v), rel(fm.w, s.w))
    assert fm.w0 == pytest.approx(s.w0, rel=1e-5, abs=1e-6)
    assert np.abs(fm.v - P["v"]).max() > 1e-4                   # it moved
    ll, conc = bref.pair_scores(s, p)
    assert bpr.computePairLogLoss(fm) == pytest.approx(ll, rel=1e-5) and abs(bpr.computePairAccuracy(fm) - conc) <= 2 / 1800
    close(bpr, fm)


# ---- 5. bit-identical --------------------------------------------------------------------------------------------------------------------------

def test_bit_identical_run_to_run(fmhip):
    """Two fresh handles and models give the same bits after 2 epochs (AdaGrad, n_neg = 3, three batches); a handle resampled at
    t = 5 and then trained from epoch 0 trains like a fresh one."""
    P = bref.make_problem(300, 32, n_neg=3)
    kw = dict(eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2], optimizer="adagrad")
    runs = []
    for detour in (False, False, True):
        bpr, fm = bref.build(fmhip, P, batch_pairs=700, **kw)
        if detour:
            bpr.resample(5)
            assert not np.array_equal(bpr.negatives(), bref.draw(P, 0)[0])
        for _ in range(2):
            bpr.learn(fm)
        runs.append((params(fm), bpr.negatives(), bpr.last_stats, get_state(fm)))
        close(bpr, fm)
    for other in runs[1:]:
        assert same(runs[0][0], other[0]) and np.array_equal(runs[0][1], other[1]) and runs[0][2] == other[2]
        assert same(runs[0][3], other[3])
    assert np.abs(runs[0][0][2] - P["v"]).max() > 1e-4


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_create_refuses_and_names_the_item(fmhip):
    """Every refusal of fmhip_bpr_create with its code and a message that names the item; afterwards the blocks and a model are
    unchanged and still train."""
    from sparkfm_amd import DataSet, _ffi
    rng = np.random.default_rng(5)
    ub, ib = rref.random_block(rng, 6, 1, 3, 0, 20), rref.random_block(rng, 9, 1, 3, 20, 50)
    mk = lambda b, **kw: DataSet(b["row_ptr"], b["col"], b["val"], np.zeros(len(b["row_ptr"]) - 1), **kw).cache()      # noqa: E731
    users, items = mk(ub), mk(ib)
    ic = np.array([0, 0, 1, 3, 5, 5, 2], np.int32)
    ii = np.array([1, 8, 4, 4, 0, 7, 2], np.int32)
    fm = fmhip.FMModel(49, 4)
    _ = fm.handle
    fm._host_fresh = False
    before = params(fm)

    def create(c, i, a=ic, b=ii, n_neg=1, n=None):
        h = C.c_void_p(7)
        rc = L().fmhip_bpr_create(0, c.handle, i.handle, len(a) if n is None else n, _ffi.ptr(a), _ffi.ptr(b), n_neg, 0, 3, C.byref(h))
        assert (rc == 0) == (h.value is not None)
        if rc == 0:
            L().fmhip_bpr_destroy(h)
        return rc, L().fmhip_last_error().decode()

    assert create(users, items)[0] == 0
    weighted, scoring, batched = mk(ib, weights=np.ones(9)), mk(ib, scoring=True), mk(ib, batch_rows=4)
    rc, msg = create(users, weighted)
    assert rc == -5 and "candidates" in msg and "weight" in msg, msg
    rc, msg = create(mk(ub, weights=np.ones(6)), items)
    assert rc == -5 and "contexts" in msg and "weight" in msg, msg
    rc, msg = create(users, scoring)
    assert rc == -5 and "candidates" in msg and "scoring" in msg, msg
    rc, msg = create(users, batched)
    assert rc == -1 and "candidates" in msg and "3 batches" in msg, msg
    shared = dict(ib, col=ib["col"].copy())
    shared["col"][shared["col"] == shared["col"].max()] = ub["col"][0]
    rc, msg = create(users, mk(shared))
    assert rc == -1 and "feature %d occurs in the contexts block and in the candidates block" % ub["col"][0] in msg, msg
    bad = ii.copy()
    bad[3] = 9
    rc, msg = create(users, items, ic, bad)
    assert rc == -1 and "interaction 3 names candidate row 9" in msg and "[0, 9)" in msg, msg
    bad = ic.copy()
    bad[5] = -1
    rc, msg = create(users, items, bad, ii)
    assert rc == -1 and "interaction 5 names context row -1" in msg and "[0, 6)" in msg, msg
    full_c, full_i = np.full(9, 4, np.int32), np.arange(9, dtype=np.int32)
    rc, msg = create(users, items, full_c, full_i)
    assert rc == -1 and "context 4 has all 9 candidate rows" in msg and "no negative" in msg, msg
    one = mk(dict(row_ptr=ib["row_ptr"][:2], col=ib["col"][:ib["row_ptr"][1]], val=ib["val"][:ib["row_ptr"][1]]))
    rc, msg = create(users, one, np.zeros(1, np.int32), np.zeros(1, np.int32))
    assert rc == -1 and "candidates block has 1 rows" in msg and "at least 2" in msg, msg
    rc, msg = create(users, items, n_neg=0)
    assert rc == -1 and "n_neg = 0" in msg, msg
    rc, msg = create(users, items, n_neg=2 ** 30 // 7 + 1)            # 7 interactions: 2 * n_pairs >= 2^31, refused before anything is sized
    assert rc == -1 and "2^31" in msg and "n_pairs" in msg, msg
    # through the Python class: the shared feature reaches the library and comes back as FmhipError
    with pytest.raises(_ffi.FmhipError, match="occurs in the contexts block") as ei:
        _ = fmhip.HipBPR.run(users, mk(shared), [[1], [], [], [], [], []]).handle
    assert ei.value.code == -1
    # a model that is too narrow; a batch out of range
    bpr = fmhip.HipBPR.run(users, items, [[1, 8], [4], [2], [4], [], [0, 7]], eta=ETA)
    with pytest.raises(_ffi.FmhipError, match="num_attribute") as ei:
        bpr.step(fmhip.FMModel(10, 4), 0)
    assert ei.value.code == -4
    with pytest.raises(_ffi.FmhipError, match="batch 1 out of range"):
        bpr.step(fm, 1)
    # nothing above touched the model or the blocks: they train
    fm._host_fresh = False
    assert same(params(fm), before)
    st = bpr.step(fm, 0)
    assert st["rows"] == 14 and st["sum_e"] == 0.0 and np.abs(fm.v - before[2]).max() > 1e-6
    # the calls are pairwise by construction: a model set to pairs, or not, trains the same, and its flag stays as it was
    from sparkfm_amd import _ffi as F
    fa, fb = fmhip.FMModel(49, 4, seed=1), fmhip.FMModel(49, 4, seed=1)
    F.check(L().fmhip_model_set_pairing(fb.handle, F.PAIRING_ADJACENT))
    bpr.step(fa, 0)
    bpr.step(fb, 0)
    assert same(params(fa), params(fb))
    for m in (fm, fa, fb):
        m.close()
    close(bpr)


# ---- 7. it learns ------------------------------------------------------------------------------------------------------------------------------------

def test_planted_preferences_are_learned(fmhip):
    """bref.planted_task(3): 30 users and 80 items, one-hot; a planted FM picks 16 items per user, 3 of them held out.  60 epochs of
    AdaGrad (eta 1.0, regw = regv = 1e-3, k = 8, n_neg = 3, batches of 128 pairs, v ~ N(0, 0.05) from seed 1003).
    The fp64 twin's held-out NDCG@10 (computed on the CPU): untrained 0.0921, popularity ranking 0.1994, trained 0.6447; its pair
    log-loss on the last epoch's training pairs 0.1990.
    Here: the trained model beats both baselines, and its own pair log-loss on the training pairs equals the twin's to rel 1e-4."""
    T = bref.planted_task(3)
    seed, k, M = 3, 8, 80
    ctx, cand, ptr, rows = bref.training_order(T["train"], M, seed, True)
    v0 = np.random.default_rng(seed + 1000).normal(0, 0.05, (k, T["n1"]))
    P = dict(seed=seed, k=k, n1=T["n1"], M=M, n_ctx=30, n_neg=3, shuffle=True, users=T["users"], items=T["items"], positives=T["train"],
             ctx=ctx, cand=cand, ptr=ptr, rows=rows, w0=0.0, w=np.zeros(T["n1"]), v=v0)
    kw = dict(eta=1.0, reg0=0.0, regw=1e-3, regv=1e-3, optimizer="adagrad", adagrad_eps=EPS, adagrad_init=0.1)
    bpr, fm = bref.build(fmhip, P, batch_pairs=128, **kw)
    users, items = bpr.contexts, bpr.candidates
    untrained = fm.computeRankingMetrics(users, items, T["held_out"], k=10, exclude=T["train"])["ndcg"]
    pop = np.bincount(np.concatenate(T["train"]), minlength=M).astype(np.float64)
    popular = bref.ndcg_at(np.tile(pop, (30, 1)), T["held_out"], T["train"])
    for _ in range(60):
        bpr.learn(fm)
    trained = fm.computeRankingMetrics(users, items, T["held_out"], k=10, exclude=T["train"])["ndcg"]
    s, p = bref.epochs(ref.State(P["w0"], P["w"], P["v"], 0.1), P, 60, 128, 1.0, 0.0, 1e-3, 1e-3, ref.Rule("logistic", True, EPS))
    ll = bref.pair_scores(s, p)[0]
    got = bpr.computePairLogLoss(fm)
    print("ndcg@10 untrained %.4f popularity %.4f trained %.4f; pair log-loss %.6f (twin %.6f)" % (untrained, popular, trained, got, ll))
    assert popular == pytest.approx(0.1994, abs=5e-5) and ll == pytest.approx(0.1990, abs=5e-5)
    assert trained > popular and trained > untrained
    assert got == pytest.approx(ll, rel=1e-4)
    close(bpr, fm)


def test_fit_and_the_fit_loop(fmhip):
    """bpr.fit(k, epochs) and FM(contexts, k, maxIteration=E).learnWith(bpr) train the same model, as wide as the larger block."""
    P = bref.make_problem(400, 8, n_neg=1)
    bpr, fm0 = bref.build(fmhip, P, batch_pairs=256, eta=ETA, regv=1e-3)
    init = (P["w0"], P["w"], P["v"])
    fm = bpr.fit(8, 2, init=init)
    assert fm.num_attribute == bpr.dimension == max(bpr.contexts.dimension, bpr.candidates.dimension) > bpr.contexts.dimension
    bpr2, _ = bref.build(fmhip, P, batch_pairs=256, eta=ETA, regv=1e-3)
    fm2 = fmhip.FM(bpr2.contexts, 8, maxIteration=2).learnWith(bpr2, init=init)
    assert fm2.num_attribute == fm.num_attribute and same(params(fm), params(fm2))
    assert bpr2.computePairLogLoss(fm2) < bpr2.computePairLogLoss(fm0)       # (the handle is made again over the re-cached contexts)
    fm2.close()
    close(bpr2)
    close(bpr, fm)
    fm0.close()


# ---- 8. include/sparkfm.hpp ----------------------------------------------------------------------------------------------------------------------

def cpp_problem():
    """The integer formulas of tests/cpp_bpr.cpp."""
    nu, ni, k, n1 = 23, 41, 8, 150

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
    positives = [[(u * 7 + t * 11) % ni for t in range(3 + u % 5)] for u in range(nu)]
    w = np.array([0.02 * ((i % 7) - 3) for i in range(n1)])
    v = np.array([[0.01 * ((f * 7 + i * 3) % 11 - 5) for i in range(n1)] for f in range(k)])
    return dict(users=block(nu, 0, 60, 7), items=block(ni, 60, 90, 11), positives=positives, k=k, n1=n1, w0=0.1, w=w, v=v)


def test_cpp_bpr_matches_python(fmhip, tmp_path):
    """tests/cpp_bpr.cpp (include/sparkfm.hpp's HipBPR) against the Python mirror over the same integer formulas: the pair log-loss
    before and after two epochs, the last draw, the sampler's statistics and every parameter, hex floats equal."""
    from sparkfm_amd import _build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_bpr")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_bpr.cpp"), "-L" + _build.LIBDIR, "-lfmhip",
                           "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = {ln.split()[0]: [float.fromhex(t) for t in ln.split()[1:]] for ln in out.stdout.decode().splitlines()}
    c = cpp_problem()
    mk = lambda b: fmhip.DataSet(b["row_ptr"], b["col"], b["val"], np.zeros(len(b["row_ptr"]) - 1), batch_rows=0)      # noqa: E731
    bpr = fmhip.HipBPR.run(mk(c["users"]), mk(c["items"]), c["positives"], n_neg=2, batch_pairs=100, seed=5, shuffle=False, eta=0.05, regw=1e-4,
                           regv=1e-4)
    fm = fmhip.FMModel(c["n1"] - 1, c["k"])
    fm.w0, fm.w, fm.v = c["w0"], c["w"], c["v"]
    before = bpr.computePairLogLoss(fm)
    bpr.learn(fm)
    bpr.learn(fm)
    assert got["before"] == [before] and got["after"] == [bpr.computePairLogLoss(fm), bpr.computePairAccuracy(fm)] and got["after"][0] < before
    assert got["neg"] == bpr.negatives().tolist()
    st = bpr.resample(1)
    assert got["attempts"] == [st["attempts"]] and got["forced"] == [st["forced"]]
    assert got["w0"] == [fm.w0] and got["w"] == fm.w.tolist() and got["v"] == fm.v.reshape(-1, order="F").tolist()
    close(bpr, fm)
