"""WARP for the BPR trainer on the GPU (include/fmhip_warp.h) against the fp64 twin of warp_ref.py: the candidates bit for bit, their
scores and the positive's to the project's pair tolerance, the kept row, the trial count and the weight against the first-violator
rule applied to the device's own scores and — on a dyadic model where fp32 is exact and ties at the threshold are planted — against
the twin's, the inverse map, the hinge step under SGD and AdaGrad, the epoch against resample + steps, the unchanged "auto" paths,
the refusals, a planted task and include/sparkfm.hpp.

The base shape is bpr_ref.make_problem's 40 contexts x 120 items with 599 interactions: 599 pairs are no multiple of the pairs a
wave (8, 4, 2, 1) or a block (32, 16, 8, 4) serves at any row width, so the last wave always holds groups without a pair."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import bpr_adaptive_ref as aref
import bpr_ref as bref
import train_ref as ref
import warp_ref as wref
from test_gpu_adagrad import EPS, get_state
from test_gpu_bpr_adaptive import N_INTER, check_inverse, close, params, problem
from topk_ref import field_rows, row_stats
from train_ref import rel, same

pytestmark = pytest.mark.gpu

REGS = (1e-3, 2e-3, 3e-3)
ETA = 0.05
M_MIXED = 0.1          # a margin at which the base problem's pairs split: some violate at once, some late, some never


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def L():
    from sparkfm_amd import _ffi
    return _ffi.load()


def wbuild(fmhip, P, n_cand, margin=1.0, batch_pairs=0, **kw):
    return bref.build(fmhip, P, batch_pairs=batch_pairs, sampler="warp", n_candidates=n_cand, margin=margin, **kw)


def twin_draw(P, t, n_cand, margin):
    return wref.draw(P, t, n_cand, margin, P["w0"], P["w"], P["v"])


def expected_from_device_scores(bpr, fm, t, margin, M):
    """The rule applied to exactly what the kernel recorded -> (rows kept, weights, N)."""
    rows, scores, pos = bpr.warp_draws(fm, t)
    n_first = wref.first_violator(scores, pos, margin)
    neg, cw = wref.choose(rows, n_first, wref.weight_table(M, bpr.n_candidates))
    return neg, cw, n_first


# ---- 1. the draws ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["base", "forced", "two_rows"])
def test_candidates_equal_the_twin(fmhip, case):
    """warp_draws' rows for C in {1, 5, 64} and t in {0, 7} against bpr_adaptive_ref.candidates, bit for bit — on the base problem, with
    a context that holds 119 of 120 rows (every candidate of its pairs is row 77) and on a 2-row candidates block — and a sub-range
    of the pairs against the same records."""
    P = problem(case)
    ctx = np.repeat(P["ctx"], P["n_neg"])
    for n_cand in (1, 5, 64):
        bpr, fm = wbuild(fmhip, P, n_cand, batch_pairs=128)
        for t in (0, 7):
            want, _, _ = aref.candidates(P["seed"], t, ctx, P["ptr"], P["rows"], P["M"], n_cand)
            rows, scores, pos = bpr.warp_draws(fm, t)
            assert rows.dtype == np.int32 and rows.shape == (len(ctx), n_cand) and np.array_equal(rows, want)
            assert scores.dtype == np.float32 and scores.shape == rows.shape and np.isfinite(scores).all()
            assert pos.dtype == np.float32 and pos.shape == (len(ctx),) and np.isfinite(pos).all()
            assert np.array_equal(rows[:, 0], bref.draw(P, t)[0])                       # candidate 0 is the uniform draw
            p1 = min(38, len(ctx))
            sub = bpr.warp_draws(fm, t, 5, p1)
            assert np.array_equal(sub[0], rows[5:p1]) and np.array_equal(sub[1], scores[5:p1]) and np.array_equal(sub[2], pos[5:p1])
            if case == "forced":
                assert (rows[ctx == 0] == 77).all()
        assert np.array_equal(bpr.negatives(), bref.draw(P, 0)[0])                      # the record mode moved no draw
        close(bpr, fm)


@pytest.mark.parametrize("k", [8, 64, 100, 200])
def test_scores_vs_fp64(fmhip, k):
    """Every candidate's device score and every positive's s+ against the fp64 score within pair_ref's tolerance of the pair — the
    bound test_gpu_bpr_adaptive.py applies — at k = 8, 64, 100, 200: groups of 8, 16, 32 and 64 lanes."""
    P = problem("base", k, seed=100 + k)
    bpr, fm = wbuild(fmhip, P, 5)
    d = twin_draw(P, 3, 5, 1.0)
    rows, scores, pos = bpr.warp_draws(fm, 3)
    assert np.array_equal(rows, d["rows"])
    err, perr = np.abs(scores.astype(np.float64) - d["scores"]), np.abs(pos.astype(np.float64) - d["pos_scores"])
    print("k = %d: max |device - fp64| / tol = %.3f (candidates), %.3f (positives)" % (k, float((err / d["tol"]).max()), float((perr / d["pos_tol"]).max())))
    assert (err <= d["tol"]).all() and (perr <= d["pos_tol"]).all()
    assert np.abs(d["pos_scores"]).max() > 0.05
    close(bpr, fm)


# ---- 2. the choice, bit for bit against the device's own scores -------------------------------------------------------------------------------

@pytest.mark.parametrize("k,batch_pairs", [(8, 0), (8, 128), (64, 0), (200, 128)])
def test_choice_is_the_first_violator_of_the_device_scores(fmhip, k, batch_pairs):
    """negatives(), trials() and pair_weights() after resample(t, fm) against wref.first_violator (fp32: the rule of
    warp_first_violator, which test_host_warp.py pins to it) and the weight table applied to the scores the kernel itself recorded —
    which looks at every candidate, so this holds whether or not the sampling kernel stops early.  C = 1, 5 (ends inside a chunk of
    4) and 64 (at k = 8: eight passes of the group); margins 0, one at which the pairs split, and one so large that every pair has
    N = 1.  The margin is moved on the handle (fmhip_warp_set): it takes effect with the next resample."""
    from sparkfm_amd import _ffi
    P = problem("base", k, seed=200 + k)
    n = N_INTER
    for n_cand in (1, 5, 64):
        bpr, fm = wbuild(fmhip, P, n_cand, batch_pairs=batch_pairs)
        seen = set()
        for t, margin in ((0, 0.0), (7, M_MIXED), (7, 1e6)):
            _ffi.check(L().fmhip_warp_set(bpr.handle, 1, margin))
            st = bpr.resample(t, fm)
            neg, cw, n_first = expected_from_device_scores(bpr, fm, t, margin, P["M"])
            assert np.array_equal(bpr.trials(), n_first) and bpr.trials().dtype == np.int32
            assert np.array_equal(bpr.negatives(), neg)
            got = bpr.pair_weights()
            assert got.dtype == np.float32 and np.array_equal(got, cw) and np.array_equal(got == 0, n_first == 0)
            assert st == dict(pairs=n, violated=int((n_first > 0).sum()), trials=int(n_first.sum())) == bpr.sample_stats
            if margin == 1e6:
                assert (n_first == 1).all() and (got == wref.weight_table(P["M"], n_cand)[1]).all()
            else:
                assert 0 < st["violated"] < n or n_cand == 64
            seen |= set(n_first.tolist())
        if n_cand == 5:
            assert seen == {0, 1, 2, 3, 4, 5}
        if n_cand == 64:
            assert max(seen) > 8 and len(seen) > 12          # violators beyond the group's first pass at k = 8
        close(bpr, fm)


# ---- 3. the choice against fp64, with exact ties at the threshold ---------------------------------------------------------------------------

def dyadic_problem(k=8, seed=7):
    """The dyadic-rational model of test_gpu_bpr_adaptive.py's exact case, rebuilt: V in multiples of 1/4 with |v| <= 1/2, w in
    multiples of 1/8, w0 = 1/4, x in {1, 1/2}, at most 3 entries a row; 40 contexts; 120 item rows drawn from 20 distinct ones, so a
    candidate's score ties exactly with other rows' — and, at margin 1/4, with thresholds.  The seed is chosen so that such ties occur."""
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


def test_choice_equals_the_twin_on_a_dyadic_model_with_ties_at_the_threshold(fmhip):
    """Every intermediate of s = yhat(i) + <q_u, q_i> and of thr = s+ - 1/4 is exact in fp32 on this model — checked here on the CPU
    by evaluating the score in float32 and in float64 — so the device's scores equal the twin's exactly, and rows, trials and weights
    must be the fp64 twin's bit for bit.  From the twin alone: candidates that tie with the threshold exactly were looked at and
    passed over (a tie is no violation)."""
    P = dyadic_problem()
    margin = 0.25
    T, _ = aref.score_table(P["w0"], P["w"], P["v"], P["users"], P["items"])
    _, qc, _ = row_stats(P["w0"], P["w"], P["v"], P["users"])
    yd, qd, _ = row_stats(P["w0"], P["w"], P["v"], P["items"])
    dot32 = np.zeros(T.shape, np.float32)
    for f in range(P["k"]):
        dot32 += qc[:, f].astype(np.float32)[:, None] * qd[:, f].astype(np.float32)[None, :]
    T32 = yd.astype(np.float32)[None, :] + dot32
    assert T32.dtype == np.float32 and (T32.astype(np.float64) == T).all()
    assert (np.abs(T) < 64).all() and (T * 256 == np.round(T * 256)).all()          # multiples of 2^-8 below 2^6: s+ - 1/4 is exact too
    for n_cand in (5, 64):
        bpr, fm = wbuild(fmhip, P, n_cand, margin=margin, batch_pairs=128)
        ties = 0
        for t in (0, 7):
            d = twin_draw(P, t, n_cand, margin)
            rows, scores, pos = bpr.warp_draws(fm, t)
            assert np.array_equal(rows, d["rows"]) and np.array_equal(scores.astype(np.float64), d["scores"])
            assert np.array_equal(pos.astype(np.float64), d["pos_scores"])
            st = bpr.resample(t, fm)
            assert np.array_equal(bpr.negatives(), d["neg"]) and np.array_equal(bpr.trials(), d["trials"])
            assert np.array_equal(bpr.pair_weights(), d["weights"])
            assert st == dict(pairs=N_INTER, violated=d["violated"], trials=d["sum_trials"])
            n_first = d["trials"][:, None]
            looked_at = np.where(n_first > 0, np.arange(n_cand)[None, :] < n_first - 1, True)
            ties += int(((d["gap"] == 0) & looked_at).sum())
        assert ties >= 3, ties
        close(bpr, fm)


# ---- 4. the inverse map ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("batch_pairs", [0, 128])
def test_inverse_map_after_a_warp_resample(fmhip, batch_pairs):
    """Every batch's device-built inverse map after resample(t, fm) against append_batch of the mapping (fmhip_bpr_debug_inverse)."""
    P = bref.make_problem(320, 16, n_inter=N_INTER, n_neg=2)
    bpr, fm = wbuild(fmhip, P, 8, margin=M_MIXED, batch_pairs=batch_pairs)
    for t in (0, 3):
        st = bpr.resample(t, fm)
        assert 0 < st["violated"] < st["pairs"] and not np.array_equal(bpr.negatives(), bref.draw(P, t)[0])
        check_inverse(bpr)
    close(bpr, fm)


# ---- 5. the step ---------------------------------------------------------------------------------------------------------------------------

# make_problem seeds found on the CPU, with the twin alone, so that no pair of the three compared batches comes within 1e-3 of the
# margin at any of the three steps (the test asserts it again on the device's own draw)
STEP_SEEDS = {(8, "sgd"): 415, (8, "adagrad"): 408, (200, "sgd"): 605, (200, "adagrad"): 605}


@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
@pytest.mark.parametrize("k", [8, 200])
def test_steps_vs_twin(fmhip, k, optimizer):
    """Steps on batches 0, 1, 2 of 5 (128 pairs a batch) after resample(2, fm) at C = 8, margin 0.1, compared after the first and after
    the third against the twin's hinge step, which starts from the DEVICE's draw (rows and weights): rel-L2 1e-4 on v and w.  The hinge
    is discontinuous, so first, from the twin alone: no pair of a compared batch lies within 1e-3 of the margin at its step.
    Statistics: rows, sum_e exactly 0, sse = 2 sum g^2 to rel 1e-5, no non-finite row."""
    P = bref.make_problem(STEP_SEEDS[(k, optimizer)], k, n_inter=N_INTER)
    kw = dict(optimizer=optimizer, eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2])
    if optimizer == "adagrad":
        kw.update(adagrad_eps=EPS, adagrad_init=0.1)
    bpr, fm = wbuild(fmhip, P, 8, margin=M_MIXED, batch_pairs=128, **kw)
    bpr.resample(2, fm)
    neg, cw, n_first = bpr.negatives(), bpr.pair_weights(), bpr.trials()
    want = expected_from_device_scores(bpr, fm, 2, M_MIXED, P["M"])
    assert np.array_equal(neg, want[0]) and np.array_equal(cw, want[1]) and np.array_equal(n_first, want[2])
    p = bref.layout(P, neg)
    s = ref.State(P["w0"], P["w"], P["v"], 0.1 if optimizer == "adagrad" else 0.0)
    rule = ref.Rule("logistic", True, EPS if optimizer == "adagrad" else None)
    # the twin's three steps, and the distance of every pair from the margin at its step
    twins, clearance, late = [], np.inf, 0
    for r0, r1 in wref.batches(len(p["y"]), 128)[:3]:
        e, d = wref.step(s, p, r0, r1, cw, M_MIXED, ETA, *REGS, rule)
        clearance = min(clearance, float(np.abs(d - M_MIXED).min()))
        late += int(((d >= M_MIXED) & (cw[r0 // 2:r1 // 2] > 0)).sum())
        twins.append((s.copy(), e))
    print("k = %d, %s: the nearest pair is %.2e from the margin; %d weighted pairs were already fixed at their step" % (k, optimizer, clearance, late))
    assert clearance > 1e-3
    assert late >= 5 and (cw[:384] == 0).sum() >= 5          # both branches of the hinge and weight 0 are in the batches
    for b in range(3):
        st = bpr.step(fm, b)
        want_s, e = twins[b]
        assert st["rows"] == 256 and st["steps"] == 1 and st["nonfinite"] == 0 and st["sum_e"] == 0.0
        assert st["sse"] == pytest.approx((e * e).sum(), rel=1e-5) and st["sse"] > 0
        if b in (0, 2):
            assert rel(fm.v, want_s.v) <= 1e-4 and rel(fm.w, want_s.w) <= 1e-4, (b, rel(fm.v, want_s.v), rel(fm.w, want_s.w))
            assert fm.w0 == pytest.approx(want_s.w0, rel=1e-4, abs=1e-6)
            if optimizer == "adagrad":
                n0, nw, nv = get_state(fm)
                assert rel(nv, want_s.nv) <= 1e-4 and rel(nw, want_s.nw) <= 1e-4 and n0 == pytest.approx(want_s.n0, rel=1e-4)
    assert np.abs(fm.v - P["v"]).max() > 1e-4                   # it moved
    assert np.array_equal(bpr.negatives(), neg)                # ... and the draw did not
    close(bpr, fm)


@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
def test_pairs_without_a_violator_give_exactly_no_gradient(fmhip, optimizer):
    """A model whose item features are all zero scores every item row w0: at margin 0 every candidate ties with the threshold, so
    every pair has N = 0 and weight 0.  A step without regularisation must then leave every parameter bit for bit — the user rows'
    q is not zero, so any residual other than an exact 0 would move the item features — with sse exactly 0."""
    P = bref.make_problem(330, 8, n_inter=N_INTER)
    P["w"][100:] = 0.0
    P["v"][:, 100:] = 0.0
    kw = dict(optimizer=optimizer, eta=ETA)
    if optimizer == "adagrad":
        kw.update(adagrad_eps=EPS, adagrad_init=0.1)
    bpr, fm = wbuild(fmhip, P, 8, margin=0.0, batch_pairs=128, **kw)
    st = bpr.resample(1, fm)
    assert st == dict(pairs=N_INTER, violated=0, trials=0) and (bpr.trials() == 0).all() and (bpr.pair_weights() == 0).all()
    assert np.array_equal(bpr.negatives(), bref.draw(P, 1)[0])                   # no violator: candidate 0's row
    # (the device holds the parameters in fp32: what was set, rounded once)
    before = (float(np.float32(P["w0"])), P["w"].astype(np.float32).astype(np.float64), P["v"].astype(np.float32).astype(np.float64))
    assert np.abs(before[2][:, :100]).max() > 0.05
    for b in (0, 4):
        s = bpr.step(fm, b)
        assert s["sse"] == 0.0 and s["sum_e"] == 0.0 and s["nonfinite"] == 0
    assert same(params(fm), before)
    if optimizer == "adagrad":          # every accumulator still at its initial value: nothing was added
        n0, nw, nv = get_state(fm)
        assert n0 == nw.min() == nw.max() == nv.min() == nv.max() and n0 == pytest.approx(0.1, rel=1e-6)
    close(bpr, fm)


# ---- 6. composition, determinism, and the unchanged paths ----------------------------------------------------------------------------------------

def test_epoch_is_resample_plus_steps_and_reruns_are_bit_identical(fmhip):
    """learn at sampler="warp", C = 4 against resample(t, fm) followed by step over the batches in order, bit for bit, for two epochs
    (the second one's candidates are scored by the model the first one trained); two fresh runs agree."""
    P = bref.make_problem(310, 16, n_inter=N_INTER, n_neg=2)
    kw = dict(eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2], optimizer="adagrad")
    runs = []
    for _ in range(2):
        bpr, fm = wbuild(fmhip, P, 4, margin=M_MIXED, batch_pairs=500, **kw)
        assert bpr.n_batches == 3
        for _ in range(2):
            bpr.learn(fm)
        runs.append((params(fm), bpr.negatives(), bpr.last_stats, get_state(fm), bpr.pair_weights(), bpr.trials()))
        close(bpr, fm)
    assert same(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2] and same(runs[0][3], runs[1][3])
    assert np.array_equal(runs[0][4], runs[1][4]) and np.array_equal(runs[0][5], runs[1][5])
    assert runs[0][2]["rows"] == 4 * N_INTER and runs[0][2]["steps"] == 3 and runs[0][2]["sum_e"] == 0.0 and runs[0][2]["sse"] > 0
    bpr, fm = wbuild(fmhip, P, 4, margin=M_MIXED, batch_pairs=500, **kw)
    drawn = []
    for t in range(2):
        st = bpr.resample(t, fm)
        assert 0 < st["violated"] < st["pairs"]
        drawn.append((bpr.negatives(), bpr.pair_weights(), bpr.trials()))
        for b in range(bpr.n_batches):
            bpr.step(fm, b, want_stats=b == 0)
    assert same(params(fm), runs[0][0]) and same(get_state(fm), runs[0][3])
    assert all(np.array_equal(x, y) for x, y in zip(drawn[1], (runs[0][1], runs[0][4], runs[0][5])))
    # the second epoch's draw read the trained model
    d1 = twin_draw(P, 1, 4, M_MIXED)
    assert not np.array_equal(drawn[1][2], d1["trials"]) and np.abs(fm.v - P["v"]).max() > 1e-4
    close(bpr, fm)


@pytest.mark.parametrize("n_cand", [1, 4])
def test_auto_handles_give_the_bits_they_gave(fmhip, n_cand):
    """Two epochs with sampler="auto" against a handle made without the keyword: parameters, AdaGrad state, statistics and draw, bit
    for bit, at one candidate (uniform) and at four (best of four) — and not WARP's."""
    P = bref.make_problem(300, 32, n_inter=N_INTER, n_neg=3)
    kw = dict(eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2], optimizer="adagrad", n_candidates=n_cand)
    out = []
    for extra in ({}, {"sampler": "auto"}, {"sampler": "auto", "margin": 0.25}, {"sampler": "warp", "margin": 0.25}):
        bpr, fm = bref.build(fmhip, P, batch_pairs=700, **kw, **extra)
        en, mg = C.c_int(-1), C.c_double(-1.0)
        assert L().fmhip_warp_get(bpr.handle, C.byref(en), C.byref(mg)) == 0
        assert (en.value, mg.value) == ((1, 0.25) if extra.get("sampler") == "warp" else (0, 1.0))
        for _ in range(2):
            bpr.learn(fm)
        out.append((params(fm), get_state(fm), bpr.last_stats, bpr.negatives()))
        close(bpr, fm)
    for other in out[1:3]:
        assert same(out[0][0], other[0]) and same(out[0][1], other[1]) and out[0][2] == other[2] and np.array_equal(out[0][3], other[3])
    assert not same(out[0][0], out[3][0])


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------

def test_refusals(fmhip):
    from sparkfm_amd import _ffi
    P = problem("base")
    bpr, fm = wbuild(fmhip, P, 3, margin=M_MIXED, batch_pairs=128)
    h = bpr.handle
    before = bpr.negatives()
    v0 = fm.v.copy()
    # no WARP draw yet: the step and the reads are refused and name the call that makes one
    with pytest.raises(_ffi.FmhipError, match="fmhip_warp_resample") as ei:
        bpr.step(fm, 0)
    assert ei.value.code == -1 and np.array_equal(fm.v, v0)
    for call in (bpr.pair_weights, bpr.trials):
        with pytest.raises(_ffi.FmhipError, match="fmhip_warp_resample"):
            call()
    # the other samplers are refused while WARP is on, before and after a draw, and leave the handle as it was
    su, sa = _ffi.BprSampleStats(), _ffi.BprAdaptiveStats()
    assert L().fmhip_bpr_resample(h, 4, C.byref(su)) == -1 and b"fmhip_warp_resample" in L().fmhip_last_error()
    assert L().fmhip_bpr_resample_adaptive(fm.handle, h, 4, C.byref(sa)) == -1 and b"fmhip_warp_resample" in L().fmhip_last_error()
    assert np.array_equal(bpr.negatives(), before) and np.array_equal(before, bref.draw(P, 0)[0])
    with pytest.raises(ValueError, match="needs a model"):
        bpr.resample(1)
    with pytest.raises(ValueError, match="use warp_draws"):
        bpr.candidate_draws(fm, 1)
    bpr.resample(1, fm)
    drawn = (bpr.negatives(), bpr.pair_weights(), bpr.trials())
    assert L().fmhip_bpr_resample(h, 4, C.byref(su)) == -1 and L().fmhip_bpr_resample_adaptive(fm.handle, h, 4, C.byref(sa)) == -1
    assert all(np.array_equal(x, y) for x, y in zip(drawn, (bpr.negatives(), bpr.pair_weights(), bpr.trials())))
    # a narrow model
    narrow = fmhip.FMModel(10, 8)
    with pytest.raises(_ffi.FmhipError, match="relational dataset has feature index .* num_attribute = 10") as ei:
        bpr.resample(1, narrow)
    assert ei.value.code == -4
    with pytest.raises(_ffi.FmhipError, match="num_attribute"):
        bpr.warp_draws(narrow, 1)
    with pytest.raises(_ffi.FmhipError, match="num_attribute"):
        bpr.step(narrow, 0)
    for p0, p1 in ((7, 7), (0, bpr.n_pairs + 1)):
        with pytest.raises(ValueError, match="non-empty range"):
            bpr.warp_draws(fm, 1, p0, p1)
    i, f = np.zeros(3, np.int32), np.zeros(3, np.float32)
    assert L().fmhip_warp_debug(fm.handle, h, 1, 4, 4, _ffi.ptr(i), _ffi.ptr(f), _ffi.ptr(f)) == -1 and b"pairs [4, 4)" in L().fmhip_last_error()
    assert L().fmhip_warp_debug(fm.handle, h, 1, 0, 1, _ffi.ptr(i), _ffi.ptr(f), None) == -1 and b"NULL" in L().fmhip_last_error()
    assert L().fmhip_warp_resample(fm.handle, h, -1, None) == -1 and b"t = -1" in L().fmhip_last_error()
    assert L().fmhip_warp_weights(h, None) == -1 and L().fmhip_warp_trials(h, None) == -1
    # none of that moved the draw (a failed resample under the narrow model stopped before the sampler ran)
    assert all(np.array_equal(x, y) for x, y in zip(drawn, (bpr.negatives(), bpr.pair_weights(), bpr.trials())))
    # a bad margin: refused, the switch, the margin and the draw stay
    en, mg = C.c_int(), C.c_double()
    for bad in (-0.5, float("nan"), float("inf"), -float("inf"), 1e300):
        assert L().fmhip_warp_set(h, 1, bad) == -1 and b"margin" in L().fmhip_last_error()
    assert L().fmhip_warp_get(h, C.byref(en), C.byref(mg)) == 0 and (en.value, mg.value) == (1, M_MIXED)
    assert L().fmhip_warp_get(h, None, None) == 0
    bpr.step(fm, 0)
    assert not np.array_equal(fm.v, v0)
    # every accepted set drops the draw; off: the handle trains as it did without WARP, and WARP's draw is refused
    _ffi.check(L().fmhip_warp_set(h, 0, M_MIXED))
    with pytest.raises(_ffi.FmhipError, match="fmhip_warp_resample"):
        bpr.pair_weights()
    assert L().fmhip_warp_resample(fm.handle, h, 1, None) == -1 and b"fmhip_warp_set" in L().fmhip_last_error()
    _ffi.check(L().fmhip_bpr_resample(h, 4, C.byref(su)))
    assert np.array_equal(bpr.negatives(), bref.draw(P, 4)[0])
    _ffi.check(L().fmhip_bpr_step(fm.handle, h, 0, ETA, 0.0, 0.0, 0.0, None))
    _ffi.check(L().fmhip_warp_set(h, 1, M_MIXED))
    with pytest.raises(_ffi.FmhipError, match="fmhip_warp_resample"):
        bpr.step(fm, 0)
    bpr.resample(2, fm)                                         # ... until the next draw
    bpr.step(fm, 0)
    narrow.close()
    close(bpr, fm)


# ---- 8. it learns -----------------------------------------------------------------------------------------------------------------------------

TWIN_HARD_3 = 0.55543861279451212      # the fp64 twin's NDCG@10 on hard_task(3) under these settings (test_host_warp.py pins 0.5554)
# twice the larger |GPU - twin| measured on the MI355X over the seeds 3 and 4 (profiles/warp.md).  Both gaps were 0: no held-out item
# changed place in any user's ranking, and NDCG is a function of the ranks alone, so the two numbers agree to the last bit
NDCG_BAND = 2 * 0.0


def run_task(fmhip, T, P, epochs, n_cand):
    kw = dict(eta=0.3, reg0=0.0, regw=1e-3, regv=1e-3, optimizer="adagrad", adagrad_eps=EPS, adagrad_init=0.1)
    bpr, fm = wbuild(fmhip, P, n_cand, margin=1.0, batch_pairs=128, **kw)
    users, items = bpr.contexts, bpr.candidates
    untrained = fm.computeRankingMetrics(users, items, T["held_out"], k=10, exclude=T["train"])["ndcg"]
    for _ in range(epochs):
        bpr.learn(fm)
    trained = fm.computeRankingMetrics(users, items, T["held_out"], k=10, exclude=T["train"])["ndcg"]
    close(bpr, fm)
    return untrained, trained


def test_harder_planted_task_is_learned_with_warp(fmhip):
    """aref.hard_task(3) — 60 users, 400 items under a popularity-skewed planted bias, 15 training and 5 held-out items a user — for 30
    epochs at C = 8, margin 1 (k = 8, n_neg = 3, batches of 128 pairs, AdaGrad eta 0.3, regw = regv = 1e-3).  The fp64 twin's held-out
    NDCG@10 (CPU; test_host_warp.py pins it): 0.5554, against 0.3064 for the best of 8 under the logistic loss and 0.1193 for the
    popularity ranking.  Asserted: the trained model beats the popularity ranking and the untrained model, and lies within
    NDCG_BAND of the twin — the hinge lets the fp32 and fp64 trajectories part, so the band is measured, not derived."""
    T = aref.hard_task(3)
    untrained, trained = run_task(fmhip, T, aref.task_problem(T, 3, 8, 3), 30, 8)
    print("hard, WARP C = 8: ndcg@10 untrained %.4f trained %.17g (twin %.17g, gap %.3e)" % (untrained, trained, TWIN_HARD_3, abs(trained - TWIN_HARD_3)))
    assert trained > 0.1193 and trained > untrained
    assert abs(trained - TWIN_HARD_3) <= NDCG_BAND


# ---- 9. include/sparkfm.hpp ---------------------------------------------------------------------------------------------------------------------

def test_cpp_warp_matches_python(fmhip, tmp_path):
    """tests/cpp_warp.cpp (include/sparkfm.hpp's HipBPR with sampler = kWarp, 4 candidates, margin 1/64) against the Python mirror over
    the integer formulas of tests/cpp_bpr.cpp: the draw, weights and trial counts after two epochs, the statistics and the draw of a
    WARP resample at t = 2, and every parameter, hex floats equal."""
    from sparkfm_amd import _build
    from test_gpu_bpr import cpp_problem
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_warp")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_warp.cpp"), "-L" + _build.LIBDIR, "-lfmhip",
                           "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = {ln.split()[0]: [float.fromhex(t) for t in ln.split()[1:]] for ln in out.stdout.decode().splitlines()}
    c = cpp_problem()
    mk = lambda b: fmhip.DataSet(b["row_ptr"], b["col"], b["val"], np.zeros(len(b["row_ptr"]) - 1), batch_rows=0)      # noqa: E731
    bpr = fmhip.HipBPR.run(mk(c["users"]), mk(c["items"]), c["positives"], n_neg=2, batch_pairs=100, seed=5, shuffle=False, eta=0.05, regw=1e-4,
                           regv=1e-4, n_candidates=4, sampler="warp", margin=1.0 / 64.0)
    fm = fmhip.FMModel(c["n1"] - 1, c["k"])
    fm.w0, fm.w, fm.v = c["w0"], c["w"], c["v"]
    bpr.learn(fm)
    bpr.learn(fm)
    assert got["candidates"] == [4] and got["margin"] == [1.0 / 64.0]
    assert got["neg"] == bpr.negatives().tolist() and got["weights"] == bpr.pair_weights().tolist() and got["trials"] == bpr.trials().tolist()
    st = bpr.resample(2, fm)
    assert (got["pairs"], got["violated"], got["sum_trials"]) == ([st["pairs"]], [st["violated"]], [st["trials"]])
    assert 0 < st["violated"] < st["pairs"] and st["trials"] > st["violated"]
    assert got["neg2"] == bpr.negatives().tolist() and got["weights2"] == bpr.pair_weights().tolist() and got["trials2"] == bpr.trials().tolist()
    assert got["w0"] == [fm.w0] and got["w"] == fm.w.tolist() and got["v"] == fm.v.reshape(-1, order="F").tolist()
    close(bpr, fm)
