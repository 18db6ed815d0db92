"""The BPR trainer, host surface (no GPU): the fp64 twin's step (bpr_ref.py) against train_ref.step on the flat expansion of the same
pairs, the sampler's properties, the Python append_batch against a hand-written case, the header against the binding, the Python-side
refusals, and the host arithmetic of fmhip_host.cpp — the positives' lists and the sampler's host twin — as a stand-alone program
under AddressSanitizer and UBSan whose printed draws are compared with the Python twin bit for bit."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bpr_ref as bref
import relational_ref as rref
import train_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the twin's step is the flat pair step -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("eps", [None, 1e-10])
@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_twin_step_is_the_flat_pair_step(loss, eps):
    """One step of the pairs [25, 175) of the base problem (n_neg = 3) by block caches with the pair residual against train_ref.step
    under Rule(loss, True, eps) on the flat expansion: 1e-12 (fp64 rounding of sums of a few dozen terms of size <= 1)."""
    P = bref.make_problem(7, 5, n_neg=3)
    neg, _, _ = bref.draw(P, 0)
    p = bref.layout(P, neg)
    a = rref.flat(p)
    assert len(p["y"]) == 2 * 3 * 600 and a["y"][:4].tolist() == [1, 0, 1, 0]
    rule = train_ref.Rule(loss, True, eps)
    s0 = train_ref.State(P["w0"], P["w"], P["v"], 0.1)
    s1 = bref.step(s0.copy(), p, 50, 350, 0.05, 1e-3, 2e-3, 3e-3, rule)
    t1 = train_ref.step(s0.copy(), a["row_ptr"], a["col"], a["val"], a["y"], 50, 350, 0.05, 1e-3, 2e-3, 3e-3, rule)
    assert np.abs(s1.v - t1.v).max() <= 1e-12 and np.abs(s1.w - t1.w).max() <= 1e-12 and abs(s1.w0 - t1.w0) <= 1e-12
    assert np.abs(s1.v - s0.v).max() > 1e-4                    # it moved
    # the contexts' residuals cancel pair by pair: their linear weights move by regw only
    users = np.unique(P["users"]["col"])
    rate = 0.05 * 2e-3
    if eps is None:
        assert np.abs(s1.w[users] - (1 - rate) * s0.w[users]).max() <= 1e-15


# ---- the sampler ---------------------------------------------------------------------------------------------------------------------

def test_no_negative_is_a_positive_and_draws_depend_on_seed_and_t():
    P = bref.make_problem(11, 4, n_neg=3)
    ctx = np.repeat(P["ctx"], 3)
    key = set((np.repeat(np.arange(P["n_ctx"]), np.diff(P["ptr"])) * P["M"] + P["rows"]).tolist())
    draws = {}
    for t in (0, 1, 7):
        neg, attempts, forced = bref.draw(P, t)
        assert neg.dtype == np.int32 and neg.shape == (1800,) and neg.min() >= 0 and neg.max() < P["M"]
        assert not any(int(u) * P["M"] + int(c) in key for u, c in zip(ctx, neg))
        assert attempts >= 1800 and forced == 0
        again = bref.draw(P, t)
        assert np.array_equal(again[0], neg) and again[1:] == (attempts, forced)
        draws[t] = neg
    assert (draws[0] != draws[1]).mean() > 0.9 and (draws[1] != draws[7]).mean() > 0.9
    other = bref.sample(P["seed"] + 1, 0, ctx, P["ptr"], P["rows"], P["M"])[0]
    assert (other != draws[0]).mean() > 0.9
    # the vectorised sampler is the step-by-step one
    for p in (0, 1, 599, 1799):
        lst = P["rows"][P["ptr"][ctx[p]]:P["ptr"][ctx[p] + 1]]
        assert bref.negative(P["seed"], p, 7, P["M"], lst)[0] == draws[7][p]


def test_draws_are_uniform_over_the_non_positives():
    """One context with 20 of 50 rows positive, 60000 pairs at a fixed seed: the counts over the 30 other rows against the uniform
    expectation 2000 by chi-square with 29 degrees of freedom.  The threshold is the p = 1e-6 quantile by the Wilson-Hilferty
    approximation df (1 - 2/(9 df) + z sqrt(2/(9 df)))^3 with z = 4.7534 (the normal's upper 1e-6 point): 81.0 for df = 29 (the exact quantile is 80.4)."""
    M, n = 50, 60000
    pos = np.arange(0, 40, 2)
    ptr, ctx = np.array([0, len(pos)]), np.zeros(n, np.int64)
    neg, attempts, forced = bref.sample(5, 3, ctx, ptr, pos, M)
    counts = np.bincount(neg, minlength=M)
    assert counts[pos].sum() == 0 and forced == 0
    free = np.setdiff1d(np.arange(M), pos)
    df = len(free) - 1
    chi2 = float(((counts[free] - n / len(free)) ** 2 / (n / len(free))).sum())
    limit = df * (1 - 2 / (9 * df) + 4.7534 * np.sqrt(2 / (9 * df))) ** 3
    assert 80.4 < limit < 81.1 and chi2 < limit, (chi2, limit)
    # a draw is accepted with probability 30 / 50: 1 / 0.6 attempts each
    assert attempts / n == pytest.approx(1 / 0.6, rel=0.02)


def test_a_context_with_one_row_left_always_gets_it():
    """M - 1 of M = 120 rows positive: every pair receives row 77; a pair is forced exactly when its 64 attempts all miss row 77
    (probability (119/120)^64 = 0.585), counted step by step with the scalar twin."""
    M, n = 120, 400
    pos = np.setdiff1d(np.arange(M), [77])
    neg, attempts, forced = bref.sample(9, 2, np.zeros(n, np.int64), np.array([0, M - 1]), pos, M)
    assert (neg == 77).all()
    by_hand = [bref.negative(9, p, 2, M, pos) for p in range(n)]
    assert all(c == 77 for c, _, _ in by_hand)
    assert forced == sum(f for _, _, f in by_hand) and attempts == sum(a for _, a, _ in by_hand)
    assert 0.45 * n < forced < 0.72 * n
    # the step up wraps: the free row below the last attempt
    pos0 = np.arange(1, M)
    assert (bref.sample(9, 2, np.zeros(50, np.int64), np.array([0, M - 1]), pos0, M)[0] == 0).all()


def test_python_append_batch_against_a_hand_written_case():
    m = [4, 1, 4, 4, 0, 4, 1, 4]
    inv = bref.append_batch(m, cut=2)
    assert inv["tj"].tolist() == [0, 1, 4] and inv["tptr"].tolist() == [0, 1, 3, 8] and inv["trow"].tolist() == [4, 1, 6, 0, 2, 3, 5, 7]
    assert inv["wt"].tolist() == [0, 1, 2, 2, 2] and inv["wbeg"].tolist() == [0, 1, 3, 5, 7] and inv["wdst"].tolist() == [0, 1, -1, -2, -3]
    assert inv["lt"].tolist() == [2] and inv["lfirst"].tolist() == [0] and inv["lcount"].tolist() == [3]
    assert inv["counts"].tolist() == [3, 5, 1, 3]


# ---- symbols -------------------------------------------------------------------------------------------------------------------------

def test_header_matches_the_binding():
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_bpr.h")).read()
    declared = set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_BPR) == {"fmhip_bpr_" + n for n in ("create", "destroy", "info", "resample", "negatives", "step", "epoch",
                                                                            "pair_logloss")}
    others = (_ffi.SYMBOLS + _ffi.SYMBOLS_EXPERIMENTAL + _ffi.SYMBOLS_TOPK + _ffi.SYMBOLS_PAIRING + _ffi.SYMBOLS_METRICS + _ffi.SYMBOLS_RANKING
              + _ffi.SYMBOLS_WEIGHTS + _ffi.SYMBOLS_RELATIONAL + _ffi.SYMBOLS_MCMC + _ffi.SYMBOLS_MCMC_TASK + _ffi.SYMBOLS_MCMC_GROUPS)
    assert not set(_ffi.SYMBOLS_BPR) & set(others) and "fmhip_bpr_debug_inverse" in _ffi.SYMBOLS_EXPERIMENTAL
    L = _ffi.load()
    for name in _ffi.SYMBOLS_BPR + ("fmhip_bpr_debug_inverse",):
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert {"fm_bpr.hip", "fmhip_bpr.hip"} <= set(_build.HIP_SOURCES) and "fm_bpr.h" in _build.HIP_DEPS
    assert "bpr" not in open(os.path.join(ROOT, "include", "fmhip.h")).read()          # fmhip.h stays as it is
    # no call through fmhip_bpr_* sets or reads the model's pairing flag
    for name in ("sparkfm_amd/csrc/fmhip_bpr.hip", "sparkfm_amd/csrc/fm_bpr.hip", "sparkfm_amd/bpr.py"):
        src = open(os.path.join(ROOT, name)).read()
        assert "set_pairing" not in src and "rule.pairing" not in src and "paired()" not in src, name
    rng_h = open(os.path.join(ROOT, "sparkfm_amd", "csrc", "mcmc_rng.h")).read()
    assert re.search(r"kStreamNegative = (\d+)", rng_h).group(1) == str(bref.STREAM_NEGATIVE) == "6"
    import sparkfm_amd
    assert sparkfm_amd.HipBPR


# ---- refusals that need no device ----------------------------------------------------------------------------------------------------------

def test_c_calls_refuse_null_arguments_without_a_device():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    h = C.c_void_p(7)
    i = np.zeros(1, np.int32)
    assert L.fmhip_bpr_create(0, None, None, 1, _ffi.ptr(i), _ffi.ptr(i), 1, 0, 0, None) == -1 and b"out is NULL" in L.fmhip_last_error()
    assert L.fmhip_bpr_create(0, None, None, 1, _ffi.ptr(i), _ffi.ptr(i), 0, 0, 0, C.byref(h)) == -1 and h.value is None
    assert b"n_neg = 0" in L.fmhip_last_error()
    assert L.fmhip_bpr_create(0, None, None, 1, _ffi.ptr(i), _ffi.ptr(i), 1, 0, 0, C.byref(h)) == -1 and b"the contexts block is NULL" in L.fmhip_last_error()
    assert L.fmhip_bpr_destroy(None) == 0
    assert L.fmhip_bpr_info(None, None, None, None, None, None) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_bpr_resample(None, 0, None) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_bpr_negatives(None, _ffi.ptr(i)) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_bpr_step(None, None, 0, 0.1, 0.0, 0.0, 0.0, None) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_bpr_epoch(None, None, 0, 0.1, 0.0, 0.0, 0.0, None, None) == -1 and b"NULL" in L.fmhip_last_error()
    out = C.c_double()
    assert L.fmhip_bpr_pair_logloss(None, None, C.byref(out), None, None) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_bpr_debug_inverse(None, 0, *[None] * 10) == -1 and b"NULL" in L.fmhip_last_error()


def test_python_refusals_and_the_training_order():
    from sparkfm_amd import DataSet, HipBPR
    users = DataSet.from_rows([(0.0, ([0], [1.0])), (0.0, ([1], [1.0])), (0.0, ([], []))], batch_rows=0)
    items = DataSet.from_rows([(0.0, ([3 + j], [1.0])) for j in range(4)], batch_rows=0)
    pos = [[2, 0, 2], [3], []]
    bpr = HipBPR.run(users, items, pos, n_neg=2, shuffle=False)
    assert bpr.inter_ctx.tolist() == [0, 0, 1] and bpr.inter_cand.tolist() == [0, 2, 3]          # sorted, de-duplicated, context-ascending
    assert (bpr.n_pairs, bpr.batch_pairs, bpr.n_batches, bpr.dimension) == (6, 6, 1, 6)
    sh = HipBPR.run(users, items, pos, seed=4, batch_pairs=2)
    perm = np.random.Generator(np.random.PCG64([4])).permutation(3)
    assert sh.inter_ctx.tolist() == np.array([0, 0, 1])[perm].tolist() and sh.inter_cand.tolist() == np.array([0, 2, 3])[perm].tolist()
    assert (sh.n_pairs, sh.n_batches) == (3, 2)
    ctx, cand, ptr, rows = bref.training_order(pos, 4, 4, True)
    assert ctx.tolist() == sh.inter_ctx.tolist() and cand.tolist() == sh.inter_cand.tolist() and ptr.tolist() == [0, 2, 3, 3]
    with pytest.raises(ValueError, match="n_neg must be >= 1"):
        HipBPR.run(users, items, pos, n_neg=0)
    with pytest.raises(ValueError, match="positives must hold one array per context"):
        HipBPR.run(users, items, pos[:2])
    with pytest.raises(ValueError, match=r"positives names a candidate row outside \[0, 4\)"):
        HipBPR.run(users, items, [[4], [], []])
    with pytest.raises(ValueError, match="context 1 has all 4 candidate rows as positives"):
        HipBPR.run(users, items, [[0], [0, 1, 2, 3], []])
    with pytest.raises(ValueError, match="no interaction"):
        HipBPR.run(users, items, [[], [], []])
    with pytest.raises(ValueError, match="at least 2"):
        HipBPR.run(users, DataSet.from_rows([(0.0, ([3], [1.0]))], batch_rows=0), [[0], [], []])
    with pytest.raises(ValueError, match="scoring-only"):
        HipBPR.run(users, DataSet.from_rows([(0.0, ([3 + j], [1.0])) for j in range(4)], batch_rows=0, scoring=True), pos)
    with pytest.raises(ValueError, match="more than one batch"):
        HipBPR.run(DataSet.from_rows([(0.0, ([0], [1.0]))] * 3, batch_rows=2), items, pos)
    with pytest.raises(ValueError, match="example weights"):
        HipBPR.run(users, DataSet.from_rows([(0.0, ([3 + j], [1.0])) for j in range(4)], batch_rows=0, weights=np.ones(4)), pos)
    with pytest.raises(ValueError, match="loss must be one of"):
        HipBPR.run(users, items, pos, loss="hinge")
    with pytest.raises(TypeError, match="contexts must be a DataSet"):
        HipBPR.run([([0], [1.0])], items, pos)


def test_fit_loop_sizes_the_model_from_the_learner():
    """FactorizationMachines.learnWith sizes its model from the dataset argument; a learner with a `dimension` of its own (HipBPR: the
    larger of its two blocks') raises it — read here without a device, through a learner that only records the model it is given."""
    from sparkfm_amd import FM, DataSet

    class Recorder:
        dimension = 41

        def learn(self, fm, dataset):
            self.n = fm.num_attribute
            raise StopIteration

    users = DataSet.from_rows([(0.0, ([0], [1.0])), (0.0, ([7], [1.0]))], batch_rows=0)
    users.cache = lambda: users                                 # (no device)
    users.unpersist = lambda: users
    rec = Recorder()
    import sparkfm_amd.fm as fm_mod
    real = fm_mod.FMModel.computeRMSE
    fm_mod.FMModel.computeRMSE = lambda self, ds: 0.0
    try:
        with pytest.raises(StopIteration):
            FM(users, 3, maxIteration=1).learnWith(rec)
    finally:
        fm_mod.FMModel.computeRMSE = real
    assert rec.n == 41


# ---- the host arithmetic under the sanitizers ------------------------------------------------------------------------------------------

def test_sampler_and_positive_lists_under_the_sanitizers(tmp_path):
    """tests/host_bpr_harness.cpp with fmhip_host.cpp under AddressSanitizer and UBSan (a program of its own; no preloading): the
    positives' lists against a brute-force build, and 400 draws — every fourth for a context with one row left — which the Python
    twin reproduces bit for bit: row, attempts and the forced flag."""
    exe = str(tmp_path / "host_bpr_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "host_bpr_harness.cpp"), os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("no sanitizer runtime for g++ in this image")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    for seed, n_ctx, M, n_inter, t in ((20261019, 12, 120, 500, 0), (5, 3, 2, 4, 7), (2 ** 40 + 3, 5, 33, 100, 4000000000)):
        r = subprocess.run([exe, str(seed), str(n_ctx), str(M), str(n_inter), "400", str(t)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env,
                           timeout=300)
        assert r.returncode == 0 and b"checks ok" in r.stdout, (seed, r.stderr.decode()[-3000:])
        lines = r.stdout.decode().splitlines()
        ptr = np.array(lines[0].split()[1:], np.int64)
        rows = np.array(lines[1].split()[1:], np.int32)
        draws = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("D ")]
        assert len(ptr) == n_ctx + 1 and len(draws) == 400
        n_forced = 0
        for p, u, c, attempts, forced in draws:
            assert bref.negative(seed, p, t, M, rows[ptr[u]:ptr[u + 1]]) == (c, attempts, forced), (seed, p)
            n_forced += forced
        assert (n_forced > 0) == (M > 2)          # one row of 120 / 33 left: most such pairs are forced; of 2, none in 64 attempts
