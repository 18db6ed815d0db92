"""The MCMC learner's tasks on the GPU (include/fmhip_mcmc_task.h, HipMCMC(task=, clip=)): a classification handle's sweeps — latent
targets from truncated normals, alpha kept at 1 — follow probit_ref.py's textbook-order sweep to the regression tests' tolerances, the
draw itself with scores past 8 on both sides, the epoch without sampling, seeds and schedules, the averaged probabilities and their
scores, the regression clamp, the planted task cut at its median, the refusals, the C++ mirror.  The shapes are test_gpu_mcmc.py's
smallest per kernel shape; the labels are cut at their median.  A comparison with the reference holds only while no accept / reject
decision of the reference was closer than 1e-6 (a last-bit difference in yhat must not flip one): every such test asserts it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mcmc_ref as R
import probit_ref as PR
from test_gpu_mcmc import assert_same_bits, cpp_rows, dataset, model, params, problem, ref_problem

pytestmark = pytest.mark.gpu
SEED = 20261019


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def binary(a):
    """the problem with its labels cut at their median: 1 above it, 0 otherwise"""
    return PR.median_cut(a)


def assert_follows(fm, mcmc, st, rtol=1e-8, atol=1e-11):
    got = mcmc.state
    np.testing.assert_allclose(fm.v, st.v, rtol=rtol, atol=atol)
    np.testing.assert_allclose(fm.w, st.w, rtol=rtol, atol=atol)
    assert fm.w0 == pytest.approx(st.w0, rel=1e-9, abs=1e-12)
    np.testing.assert_allclose(got["lambda"], st.lam, rtol=1e-9)
    np.testing.assert_allclose(got["mu"], st.mu, rtol=1e-9)
    assert got["alpha"] == 1.0 == mcmc.last_stats["alpha"] == st.alpha


# ---- 1. sampled sweeps against the reference --------------------------------------------------------------------------------------

SAMPLED = [("lds", 2000, 25, 3, {}), ("lds", 10001, 300, 2, {}), ("onehot", 9000, (300, 200), 4, {"FMHIP_ALS_LEVELS": "1"})]


@pytest.mark.parametrize("kind,n_rows,shape,k,env", SAMPLED, ids=["lds-walk", "workgroup-walk", "levels"])
def test_sampled_sweeps_follow_the_reference(fmhip, monkeypatch, kind, n_rows, shape, k, env):
    """Three epochs — the first trains on +-1, the next two on drawn targets — against probit_ref: parameters to rtol 1e-8 / atol 1e-11,
    lambda and mu to 1e-9 (the sampled regression test's tolerances: the same fp64 arithmetic plus a draw that is a few ulp off), alpha
    exactly 1, the latent targets to 1e-9, train_rmse that of the latent residuals.  Both branches of the draw are taken."""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    a = binary(problem(kind, n_rows, shape, k))
    ds = dataset(fmhip, a)
    fm = model(fmhip, a, k)
    mcmc = fmhip.HipMCMC.run(seed=SEED, task="classification")
    st, p = R.State(a["w0"], a["w"], a["v"]), ref_problem(a)
    margin, right = np.inf, []
    for it in range(3):
        mcmc.learn(fm, ds)
        o = PR.epoch(st, p, seed=SEED)
        margin = min(margin, o["margin"])
        assert mcmc.last_stats["train_rmse"] == pytest.approx(np.sqrt(o["sse"] / n_rows), rel=1e-9) and mcmc.last_stats["iterations"] == it + 1
        ystar = mcmc.latent_targets()
        np.testing.assert_allclose(ystar, o["ystar"], rtol=0, atol=1e-9)
        if it == 0:
            assert np.array_equal(ystar, np.where(a["y"] > 0, 1.0, -1.0))
        else:
            right.append(float(np.mean(-o["s"] * o["yhat"] > 0)))
            assert o["attempts"].max() > 1
    print("smallest decision margin %.3e  share of rows with a > 0: %s  max |dv| %.3e" % (margin, right, np.abs(fm.v - st.v).max()))
    assert margin >= 1e-6, margin
    assert all(0.1 < r < 0.9 for r in right)
    assert_follows(fm, mcmc, st)
    n1 = a["n1"]
    assert np.array_equal(fm.v[:, n1 - 1], a["v"][:, n1 - 1]) and fm.w[n1 - 1] == a["w"][n1 - 1]      # quirk Q1
    mcmc.close()
    fm.close()
    ds.unpersist()


# ---- 2. the draw itself ------------------------------------------------------------------------------------------------------------

def test_the_draw_with_scores_past_eight_on_both_sides(fmhip):
    """After the first epoch the model is set to weights scaled until |yhat| passes 8 on both sides (some rows empty: yhat = w0), and the
    second epoch draws around those scores: every y* has its label's sign (a = -s yhat from below -8 to above 8: the normal branch deep
    inside its support, the exponential proposal far in the tail), and yhat + s z is the reference's to 1e-9."""
    from helpers import random_problem
    k = 3
    a = random_problem(911, 1500, 25, k, 1, 12, empty_rows=(0, 7, 700, 1499))
    a = binary(a)
    big = random_problem(912, 4, 25, k, 1, 2, scale=0.7)
    ds = dataset(fmhip, a)
    fm = model(fmhip, a, k)
    mcmc = fmhip.HipMCMC.run(seed=SEED, task="classification")
    st, p = R.State(a["w0"], a["w"], a["v"]), ref_problem(a)
    mcmc.learn(fm, ds)
    PR.epoch(st, p, seed=SEED)
    fm.w0, fm.w, fm.v = 0.3, big["w"], big["v"]
    st.w0, st.w, st.v = 0.3, big["w"].copy(), big["v"].copy()
    mcmc.learn(fm, ds)
    o = PR.epoch(st, p, seed=SEED)
    ystar = mcmc.latent_targets()
    lo = -o["s"] * o["yhat"]
    print("a from %.2f to %.2f, most attempts %d, margin %.3e, max |dy*| %.3e" % (lo.min(), lo.max(), o["attempts"].max(), o["margin"],
                                                                                 np.abs(ystar - o["ystar"]).max()))
    assert o["yhat"].min() < -8.0 and o["yhat"].max() > 8.0 and lo.min() < -8.0 and lo.max() > 8.0
    assert o["margin"] >= 1e-6, o["margin"]
    assert (np.sign(ystar) == o["s"]).all() and (ystar != 0).all()
    np.testing.assert_allclose(ystar, o["ystar"], rtol=0, atol=1e-9)
    empty = np.flatnonzero(np.diff(a["row_ptr"]) == 0)
    assert len(empty) == 4 and (o["yhat"][empty] == 0.3).all()
    mcmc.close()
    fm.close()
    ds.unpersist()


# ---- 3. without sampling -------------------------------------------------------------------------------------------------------------

def test_without_sampling_the_targets_are_the_expected_values(fmhip):
    """sample=False: three epochs against the reference's expected-value epoch (z = E[z | z > a]), the same tolerances; no draw at all —
    the state stays what it was set to."""
    k = 3
    a = binary(problem("lds", 2000, 25, k))
    ds = dataset(fmhip, a)
    fm = model(fmhip, a, k)
    mcmc = fmhip.HipMCMC.run(seed=SEED, task="classification", sample=False)
    lam, mu = np.array([0.5, 2.0, 3.0, 4.0]), np.array([0.0, 0.01, -0.02, 0.0])
    mcmc.state = (1.0, lam, mu)
    st, p = R.State(a["w0"], a["w"], a["v"]), ref_problem(a)
    st.lam, st.mu = lam.copy(), mu.copy()
    for it in range(3):
        mcmc.learn(fm, ds)
        o = PR.epoch(st, p, seed=SEED, sample=False)
        np.testing.assert_allclose(mcmc.latent_targets(), o["ystar"], rtol=0, atol=1e-9)
        assert mcmc.last_stats["train_rmse"] == pytest.approx(np.sqrt(o["sse"] / 2000), rel=1e-9)
    assert_follows(fm, mcmc, st)
    got = mcmc.state
    assert got["alpha"] == 1.0 and np.array_equal(got["lambda"], lam) and np.array_equal(got["mu"], mu) and got["iterations"] == 3
    assert np.abs(fm.v - a["v"]).max() > 1e-3
    # another seed: the same bits (nothing is drawn)
    fm2 = model(fmhip, a, k)
    other = fmhip.HipMCMC.run(seed=5, task="classification", sample=False)
    other.state = (1.0, lam, mu)
    for _ in range(3):
        other.learn(fm2, ds)
    assert_same_bits(params(fm), params(fm2))
    for h in (mcmc, other, fm, fm2):
        h.close()
    ds.unpersist()


# ---- 4. determinism ----------------------------------------------------------------------------------------------------------------

def test_seeds_and_schedules(fmhip, monkeypatch):
    k = 4
    a = binary(problem("onehot", 9000, (300, 200), k))
    ds = dataset(fmhip, a)

    def run(seed, levels, **kw):
        monkeypatch.setenv("FMHIP_ALS_LEVELS", levels)
        fm = model(fmhip, a, k)
        mcmc = fmhip.HipMCMC.run(seed=seed, **kw)
        for _ in range(2):
            mcmc.learn(fm, ds)
        out = params(fm) + (mcmc.latent_targets(), mcmc.state)
        mcmc.close()
        fm.close()
        return out
    one, again, other, flat = run(5, "1", task="classification"), run(5, "1", task="classification"), run(6, "1", task="classification"), run(5, "0", task="classification")
    assert_same_bits(one, again)
    assert np.array_equal(one[3], again[3]) and np.array_equal(one[4]["lambda"], again[4]["lambda"])
    assert (one[3] != other[3]).all() and (np.sign(one[3]) == np.sign(other[3])).all() and (one[2][:, :-1] != other[2][:, :-1]).all()
    # the latent draw does not depend on the schedule: the level schedule against the sequential walk, equal bits (9000 rows: the LDS walk)
    assert_same_bits(one, flat)
    assert np.array_equal(one[3], flat[3])
    # a regression handle is fmhip_mcmc_create's, bit for bit: HipMCMC (fmhip_mcmc_create_task with the default task), the call with a NULL task
    from sparkfm_amd import _ffi
    L = _ffi.load()
    opts = _ffi.McmcOpts()
    L.fmhip_mcmc_opts_default(C.byref(opts))
    opts.seed = 5

    def raw(create):
        fm = model(fmhip, a, k)
        h = C.c_void_p()
        _ffi.check(create(fm.handle, ds.handle, C.byref(h)))
        labels = np.empty(9000)
        _ffi.check(L.fmhip_mcmc_latent_targets(h, _ffi.ptr(labels)))
        assert np.array_equal(labels, a["y"])                   # before the first epoch: the labels
        for _ in range(2):
            _ffi.check(L.fmhip_mcmc_epoch(h, None))
            fm._device_updated()
        _ffi.check(L.fmhip_mcmc_latent_targets(h, _ffi.ptr(labels)))
        assert np.array_equal(labels, a["y"])                   # a regression handle: the labels
        out = params(fm)
        L.fmhip_mcmc_destroy(h)
        fm.close()
        return out
    plain = raw(lambda m, d, h: L.fmhip_mcmc_create(m, d, None, C.byref(opts), h))
    null_task = raw(lambda m, d, h: L.fmhip_mcmc_create_task(m, d, None, C.byref(opts), None, h))
    regression = run(5, "1")
    assert_same_bits(plain, null_task)
    assert_same_bits(plain, regression)
    assert np.array_equal(regression[3], a["y"]) and regression[4]["alpha"] != 1.0
    assert (plain[2][:, :-1] != one[2][:, :-1]).all()           # ... and not the classification handle's
    ds.unpersist()


# ---- 5. averaged probabilities --------------------------------------------------------------------------------------------------------

def auc_of(p, y):
    """ROC AUC with ties counting one half, scores compared as float32 (fmhip_auc's convention)"""
    s, t = np.asarray(p, np.float32), np.asarray(y) > 0
    pos, neg = s[t], s[~t]
    return float(((pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()) / (len(pos) * len(neg)))


def test_averaged_probabilities(fmhip):
    """Four epochs with a test set: predictions() is the mean of the four draws' Phi(yhat) (probit_ref) to 1e-8, last_predictions() the
    fourth draw's; with burn_in = 2 the mean of the last two.  computeLogLoss / computeAccuracy / computeAUC are numpy's on those."""
    from helpers import random_problem
    k = 3
    a = binary(problem("lds", 2000, 25, k))
    b = random_problem(31, 500, 25, k, 0, 12)
    b["y"] = (b["y"] > 0).astype(np.float64)
    ds, test = dataset(fmhip, a), dataset(fmhip, b)
    st, p, pt = R.State(a["w0"], a["w"], a["v"]), ref_problem(a), ref_problem(b)
    draws, margin = [], np.inf
    for _ in range(4):
        margin = min(margin, PR.epoch(st, p, seed=9)["margin"])
        draws.append(PR.normal_cdf(R.predict(st.w0, st.w, st.v, pt)))
    assert margin >= 1e-6, margin
    for burn_in in (0, 2):
        fm = model(fmhip, a, k)
        mcmc = fmhip.HipMCMC.run(seed=9, test=test, burn_in=burn_in, task="classification")
        for _ in range(4):
            mcmc.learn(fm, ds)
        kept = np.mean(draws[burn_in:], axis=0)
        mean, last = mcmc.predictions(), mcmc.last_predictions()
        assert mcmc.draws == 4 - burn_in
        np.testing.assert_allclose(mean, kept, rtol=0, atol=1e-8)
        np.testing.assert_allclose(last, draws[3], rtol=0, atol=1e-8)
        assert (mean > 0).all() and (mean < 1).all() and np.abs(mean - 0.5).max() > 0.1
        assert mcmc.computeLogLoss() == pytest.approx(PR.logloss(mean, b["y"]), abs=1e-12)
        assert mcmc.computeLogLoss() == pytest.approx(PR.logloss(kept, b["y"]), abs=1e-7)
        assert mcmc.computeAccuracy() == PR.accuracy(mean, b["y"])
        assert mcmc.computeAUC() == pytest.approx(auc_of(mean, b["y"]), abs=1e-12)
        with pytest.raises(ValueError, match="computeLogLoss"):
            mcmc.computeRMSE()
        # the model holds the last draw: its score is the probit score (fp32 scoring)
        np.testing.assert_allclose(PR.normal_cdf(fm.predict(test)), draws[3], rtol=0, atol=1e-4)
        mcmc.close()
        fm.close()
    ds.unpersist()
    test.unpersist()


# ---- 6. the regression clamp ------------------------------------------------------------------------------------------------------------

def test_clip_clamps_every_draw(fmhip):
    """Regression, four epochs, clip = (lo, hi) inside the draws' range: predictions() is the mean of the reference's CLAMPED draws to 1e-8
    (not the clamped mean), last_predictions() the clamped fourth draw.  The clamp touches the test rows only: the parameters are an
    unclipped run's bits, and so are the predictions under a range wider than every draw, and under clip="labels" when no draw leaves it."""
    from helpers import random_problem
    k = 3
    a = problem("lds", 2000, 25, k)
    b = random_problem(31, 500, 25, k, 0, 12)
    ds, test = dataset(fmhip, a), dataset(fmhip, b)
    st, p, pt = R.State(a["w0"], a["w"], a["v"]), ref_problem(a), ref_problem(b)
    draws = []
    for _ in range(4):
        R.epoch(st, p, seed=9)
        draws.append(R.predict(st.w0, st.w, st.v, pt))
    draws = np.array(draws)
    lo, hi = float(np.quantile(draws, 0.2)), float(np.quantile(draws, 0.8))
    clamped = np.clip(draws, lo, hi)
    assert np.abs(clamped.mean(0) - np.clip(draws.mean(0), lo, hi)).max() > 1e-3       # the order of clamp and mean matters here

    def run(clip):
        fm = model(fmhip, a, k)
        mcmc = fmhip.HipMCMC.run(seed=9, test=test, clip=clip)
        for _ in range(4):
            mcmc.learn(fm, ds)
        out = params(fm) + (mcmc.predictions(), mcmc.last_predictions(), mcmc.computeRMSE())
        mcmc.close()
        fm.close()
        return out
    none, clip, wide = run(None), run((lo, hi)), run((draws.min() - 1.0, draws.max() + 1.0))
    np.testing.assert_allclose(clip[3], clamped.mean(0), rtol=0, atol=1e-8)
    np.testing.assert_allclose(clip[4], clamped[3], rtol=0, atol=1e-8)
    assert clip[3].min() >= lo and clip[3].max() <= hi and (clip[4] == lo).any() and (clip[4] == hi).any()
    assert clip[5] == pytest.approx(R.rmse(clamped.mean(0), b["y"]), abs=1e-8)
    np.testing.assert_allclose(none[3], draws.mean(0), rtol=0, atol=1e-8)
    assert_same_bits(none, clip)
    assert_same_bits(none, wide)
    assert np.array_equal(none[3], wide[3]) and np.array_equal(none[4], wide[4])
    labels = run("labels")
    np.testing.assert_allclose(labels[3], np.clip(draws, a["y"].min(), a["y"].max()).mean(0), rtol=0, atol=1e-8)
    ds.unpersist()
    test.unpersist()


# ---- 7. it does what it is for ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2])
def test_planted_classification_task(fmhip, seed):
    """The planted two-field task of test_planted_rating_task (task seed 2026, 600 train / 300 test rows, model k = 4) with its labels cut
    at the train median: 15 burn-in epochs + 25 kept.  The library's averaged and last-draw test log-loss are probit_ref's to 1e-6, the
    averaged one is below the last draw's, and the averaged accuracy is above the majority class's share (0.537).  probit_ref itself,
    run on the CPU with these Philox streams, gave averaged / last log-loss 0.4466 / 0.7272 (ratio 0.614; accuracy 0.797 / 0.740) for
    seed 1 and 0.4285 / 0.6538 (0.655; 0.800 / 0.747) for seed 2; seed 3 gave 0.4467 / 0.7636 (0.585) — all inside the 0.9 a seed had
    to show to be kept; the most attempts a row's draw took was 12, the smallest decision margin 1.9e-5."""
    tr, te = PR.median_cut(*R.planted_task(2026))
    n1, k = tr["n1"], 4
    init = dict(n1=n1, w0=0.0, w=np.zeros(n1), v=np.random.default_rng(5).normal(0, 0.01, (k, n1)))
    ds, test = dataset(fmhip, tr), dataset(fmhip, te)
    fm = model(fmhip, init, k)
    mcmc = fmhip.HipMCMC.run(seed=seed, test=test, burn_in=15, task="classification")
    for _ in range(40):
        mcmc.learn(fm, ds)
    avg, last = mcmc.computeLogLoss(), PR.logloss(mcmc.last_predictions(), te["y"])
    st, p, pt = R.State(init["w0"], init["w"], init["v"]), ref_problem(tr), ref_problem(te)
    acc, margin = np.zeros(pt.n_rows), np.inf
    for it in range(40):
        margin = min(margin, PR.epoch(st, p, seed=seed)["margin"])
        ref_last = PR.normal_cdf(R.predict(st.w0, st.w, st.v, pt))
        if it >= 15:
            acc += ref_last
    ref_avg, ref_last = PR.logloss(acc / 25, te["y"]), PR.logloss(ref_last, te["y"])
    majority = max(float(np.mean(te["y"] > 0)), float(np.mean(te["y"] <= 0)))
    print("log-loss averaged %.6f (ref %.6f)  last %.6f (ref %.6f)  ratio %.3f  accuracy %.4f (majority %.4f)  AUC %.4f  margin %.2e"
          % (avg, ref_avg, last, ref_last, avg / last, mcmc.computeAccuracy(), majority, mcmc.computeAUC(), margin))
    assert mcmc.draws == 25 and margin >= 1e-6
    assert ref_avg <= 0.9 * ref_last
    assert abs(avg - ref_avg) <= 1e-6 and abs(last - ref_last) <= 1e-6
    assert avg < last
    assert mcmc.computeAccuracy() > majority
    assert mcmc.state["alpha"] == 1.0
    for h in (mcmc, fm):
        h.close()
    ds.unpersist()
    test.unpersist()


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_model_unchanged(fmhip):
    """A classification handle refuses what the regression handle refuses, in the same words (test_gpu_mcmc.py's list), the model unchanged —
    the task belongs to the handle: a model set to the logistic loss is still refused."""
    from helpers import random_problem
    from sparkfm_amd import _ffi
    L = _ffi.load()
    k = 3
    a = binary(problem("lds", 2000, 25, k))
    fm = model(fmhip, a, k)
    start = params(fm)

    def refused(train, code, words, test=None):
        said = []
        for task in ("regression", "classification"):
            mcmc = fmhip.HipMCMC.run(test=test, task=task)
            with pytest.raises(_ffi.FmhipError, match=words) as err:
                mcmc.learn(fm, train)
            assert err.value.code == code
            said.append(str(err.value))
            assert_same_bits(params(fm), start)
            mcmc.close()
        assert said[0] == said[1]
    ok = dataset(fmhip, a)
    multi = dataset(fmhip, a, batch_rows=700)
    refused(multi, -5, "ALS walks the whole-dataset transpose")
    weighted = dataset(fmhip, a, weights=np.ones(2000))
    refused(weighted, -5, "ALS is derived for the squared loss of unweighted rows")
    dup = fmhip.DataSet.from_rows([(1.0, ([0, 2, 2], [1.0, 2.0, 0.5])), (0.0, ([1], [1.0]))]).cache()
    refused(dup, -5, "twice")
    scoring = dataset(fmhip, a, scoring=True)
    refused(scoring, -5, "scoring only")
    h = C.c_void_p()
    task = _ffi.McmcTaskOpts(_ffi.MCMC_CLASSIFICATION, 0, 0.0, 0.0)
    assert L.fmhip_mcmc_create_task(fm.handle, ok.handle, scoring.handle, None, C.byref(task), C.byref(h)) == -5 and h.value is None and b"fp64" in L.fmhip_last_error()
    refused(ok, -5, "fp64", test=multi)
    b = random_problem(3, 50, 40, k, 1, 5)
    b["col"][0] = 39
    wide = dataset(fmhip, b)
    refused(ok, -1, "test set has feature index 39", test=wide)
    assert L.fmhip_model_set_loss(fm.handle, _ffi.LOSS_LOGISTIC) == 0
    refused(ok, -5, "ALS is derived for the squared loss: this model trains under the logistic loss")
    assert L.fmhip_model_set_loss(fm.handle, _ffi.LOSS_SQUARED) == 0 and L.fmhip_model_set_pairing(fm.handle, _ffi.PAIRING_ADJACENT) == 0
    refused(ok, -5, "pairs of rows")
    assert L.fmhip_model_set_pairing(fm.handle, _ffi.PAIRING_NONE) == 0
    # the task's own refusals, with a model and a dataset at hand
    for bad, words in ((_ffi.McmcTaskOpts(7, 0, 0.0, 0.0), b"unknown task"), (_ffi.McmcTaskOpts(1, 1, 0.0, 1.0), b"regression task"),
                       (_ffi.McmcTaskOpts(0, 1, 1.0, 1.0), b"clip range")):
        assert L.fmhip_mcmc_create_task(fm.handle, ok.handle, None, None, C.byref(bad), C.byref(h)) == -1 and h.value is None and words in L.fmhip_last_error()
    # ... and afterwards it trains; a classification run has no RMSE
    mcmc = fmhip.HipMCMC.run(task="classification", test=ok)
    mcmc.learn(fm, ok)
    assert np.abs(fm.v - start[2]).max() > 1e-3
    with pytest.raises(ValueError, match="computeLogLoss"):
        mcmc.computeRMSE()
    assert 0.0 < mcmc.computeLogLoss() < 2.0
    mcmc.close()
    fm.close()
    for d in (ok, multi, weighted, dup, scoring, wide):
        d.unpersist()


# ---- 9. the C++ mirror ----------------------------------------------------------------------------------------------------------------------

def test_cpp_mcmc_probit_matches_python(fmhip, tmp_path):
    """tests/cpp_mcmc_probit.cpp (include/sparkfm.hpp's HipMCMC with the classification task) against the Python mirror over cpp_mcmc.cpp's
    integer formulas, labels cut at 0.5: three sweeps with a test set and one burn-in epoch — parameters, state, latent targets, the
    averaged and the last probabilities, hex floats equal; then a regression run with a clip."""
    from sparkfm_amd import _build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_mcmc_probit")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_mcmc_probit.cpp"), "-L" + _build.LIBDIR, "-lfmhip",
                           "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.decode().splitlines()}
    hexes = lambda name: [float.fromhex(t) for t in got[name]]      # noqa: E731
    n1, k = 40, 3
    a = dict(n1=n1, w0=0.1, w=np.array([0.02 * ((i % 7) - 3) for i in range(n1)]),
             v=np.array([[0.01 * ((f * 7 + i * 3) % 11 - 5) for i in range(n1)] for f in range(k)]))
    tr, te = cpp_rows(400, 0), cpp_rows(100, 1000)
    for d in (tr, te):
        d["y"] = (d["y"] > 0.5).astype(np.float64)
    ds, test = dataset(fmhip, tr), dataset(fmhip, te)
    fm = model(fmhip, a, k)
    mcmc = fmhip.HipMCMC.run(seed=12, test=test, burn_in=1, task="classification")
    for _ in range(3):
        mcmc.learn(fm, ds)
    st = mcmc.state
    assert hexes("w0") == [fm.w0] and hexes("w") == fm.w.tolist() and hexes("v") == fm.v.reshape(-1, order="F").tolist()
    assert hexes("alpha") == [st["alpha"], mcmc.last_stats["alpha"]] == [1.0, 1.0] and hexes("lambda") == st["lambda"].tolist() and hexes("mu") == st["mu"].tolist()
    assert hexes("ystar") == mcmc.latent_targets().tolist()
    assert hexes("mean") == mcmc.predictions().tolist() and hexes("last") == mcmc.last_predictions().tolist()
    assert hexes("logloss")[0] == pytest.approx(mcmc.computeLogLoss(), rel=1e-12) and hexes("accuracy") == [mcmc.computeAccuracy()]
    assert got["draws"] == ["2", "3"] and got["rmse_refused"] == ["1"]
    assert np.abs(fm.v - a["v"]).max() > 1e-3
    mcmc.close()
    fm.close()
    # the regression run with a clip, from the same start
    fm = model(fmhip, a, k)
    tr["y"], te["y"] = cpp_rows(400, 0)["y"], cpp_rows(100, 1000)["y"]
    ds2, test2 = dataset(fmhip, tr), dataset(fmhip, te)
    mcmc = fmhip.HipMCMC.run(seed=12, test=test2, clip=(0.3, 0.7))
    for _ in range(2):
        mcmc.learn(fm, ds2)
    assert hexes("clip_mean") == mcmc.predictions().tolist() and hexes("clip_w") == fm.w.tolist()
    labels = fmhip.HipMCMC.run(seed=12, test=test2, clip="labels")
    fm2 = model(fmhip, a, k)
    for _ in range(2):
        labels.learn(fm2, ds2)
    assert hexes("labels_mean") == labels.predictions().tolist()
    for h in (mcmc, labels, fm, fm2):
        h.close()
    for d in (ds, test, ds2, test2):
        d.unpersist()
