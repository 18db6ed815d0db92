"""The BPR trainer's weighted proposal, host surface (no GPU): the header against the binding and the exported symbols, the alias
table's implied probabilities, the twin's draws (their distribution, one row left, equal weights), the refusals that need no device,
the host arithmetic under the sanitizers against the Python twin, and the twin's held-out NDCG on the harder planted task."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import bpr_adaptive_ref as aref
import bpr_proposal_ref as pref
import bpr_ref as bref
import train_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"fmhip_proposal_" + n for n in ("set", "get", "table")}


# ---- symbols -------------------------------------------------------------------------------------------------------------------------

def test_header_matches_the_binding_and_the_library():
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_proposal.h")).read()
    declared = set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_PROPOSAL) == NAMES
    others = (_ffi.SYMBOLS + _ffi.SYMBOLS_EXPERIMENTAL + _ffi.SYMBOLS_TOPK + _ffi.SYMBOLS_PAIRING + _ffi.SYMBOLS_METRICS + _ffi.SYMBOLS_RANKING
              + _ffi.SYMBOLS_WEIGHTS + _ffi.SYMBOLS_RELATIONAL + _ffi.SYMBOLS_MCMC + _ffi.SYMBOLS_MCMC_TASK + _ffi.SYMBOLS_MCMC_GROUPS
              + _ffi.SYMBOLS_MCMC_RELATIONAL + _ffi.SYMBOLS_BPR + _ffi.SYMBOLS_BPR_ADAPTIVE + _ffi.SYMBOLS_WARP + _ffi.SYMBOLS_FTRL + _ffi.SYMBOLS_REDRAW
              + _ffi.SYMBOLS_SGDA)
    assert not NAMES & set(others) and not [n for n in others if n.startswith("fmhip_proposal_")]
    L = _ffi.load()
    for name in _ffi.SYMBOLS_PROPOSAL:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int, name
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert set(re.findall(r"\bT (fmhip_proposal_[a-z0-9_]+)", out)) == NAMES
    assert os.path.join("..", "..", "include", "fmhip_proposal.h") in _build.HIP_DEPS
    # the header states what WARP's rank estimate means under a weighted proposal
    assert "rank among proposal-weighted items" in hdr and "assumes a uniform proposal" in hdr
    # the C++ wrapper carries the keyword
    hpp = open(os.path.join(ROOT, "include", "sparkfm.hpp")).read()
    assert "fmhip_proposal.h" in hpp and "kPopularity" in hpp and "fmhip_proposal_set" in hpp


def test_c_calls_refuse_null_handles_without_a_device():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    w = np.ones(4)
    flag = C.c_int(-5)
    assert L.fmhip_proposal_set(None, _ffi.ptr(w)) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error()
    assert L.fmhip_proposal_set(None, None) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error()
    assert L.fmhip_proposal_get(None, C.byref(flag)) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error()
    assert flag.value == -5
    assert L.fmhip_proposal_table(None, None, None) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error()


# ---- the table -------------------------------------------------------------------------------------------------------------------------

def popularity_counts(M):
    P = bref.make_problem(77, 8, M=M, n_inter=600)
    return pref.popularity(P)


@pytest.mark.parametrize("name,weights", [
    ("equal", np.ones(97)),
    ("dominant", np.array([1e6] + [1.0] * 119)),
    ("two", np.array([3.0, 1.0])),
    ("two_equal", np.array([2.5, 2.5])),
    ("popularity", popularity_counts(120)),
    ("power_law_4096", (1.0 + np.arange(4096)) ** -1.1),
])
def test_table_gives_every_row_its_share(name, weights):
    """The probability the table implies for row i — (thresh_i + the sum over the buckets j != i with alias_j = i of
    2^32 - thresh_j) / (M 2^32), a bucket with alias_j = j counting as 2^32 — in exact rational arithmetic against w_i / sum(w) to
    within 2^-30: each of the M <= 4096 thresholds is floored by less than 2^-32 of a bucket of mass 1 / M, and Vose's fp64
    updates err by a few 2^-53 of a bucket each."""
    thresh, alias = pref.alias_table(weights)
    M = len(weights)
    assert thresh.dtype == np.uint32 and alias.dtype == np.int32 and len(thresh) == len(alias) == M
    assert ((alias >= 0) & (alias < M)).all()
    got = pref.implied(thresh, alias)
    assert sum(got) == 1
    total = sum(Fraction(float(x)) for x in weights)
    worst = max(abs(g - Fraction(float(x)) / total) for g, x in zip(got, weights))
    print("%s: max |implied - w / sum| = 2^%.1f" % (name, np.log2(float(worst)) if worst else -np.inf))
    assert worst <= Fraction(1, 2 ** 30)
    if name in ("equal", "two_equal"):
        assert (alias == np.arange(M)).all() and (thresh == 2 ** 32 - 1).all()       # no bucket is redirected
    if name == "dominant":
        assert alias[0] == 0 and (alias[1:] == 0).all() and (thresh[1:] < 2 ** 32 * 120 / 1e6).all()


# ---- the draws ---------------------------------------------------------------------------------------------------------------------------

def test_draws_follow_the_weights_over_the_non_positives():
    """One context with 20 of 50 rows positive, 60000 pairs, weights (1 + i)^0.75, at a seed chosen on the twin and fixed: the counts
    over the 30 free rows against the weights renormalised over those rows by chi-square with 29 degrees of freedom, at the
    Wilson-Hilferty p = 1e-6 threshold test_host_bpr.py uses (81.0).  No row is a positive and no pair is forced."""
    M, n = 50, 60000
    pos = np.arange(0, 40, 2)
    w = (1.0 + np.arange(M)) ** 0.75
    ptr, ctx = np.array([0, len(pos)]), np.zeros(n, np.int64)
    neg, attempts, forced = pref.sample(5, 3, ctx, ptr, pos, M, pref.alias_table(w))
    counts = np.bincount(neg, minlength=M)
    assert counts[pos].sum() == 0 and forced == 0
    free = np.setdiff1d(np.arange(M), pos)
    expect = n * w[free] / w[free].sum()
    df = len(free) - 1
    chi2 = float(((counts[free] - expect) ** 2 / expect).sum())
    limit = df * (1 - 2 / (9 * df) + 4.7534 * np.sqrt(2 / (9 * df))) ** 3
    print("chi2 = %.2f (limit %.2f)" % (chi2, limit))
    assert 80.4 < limit < 81.1 and chi2 < limit, (chi2, limit)
    # the uniform expectation is far off: the test can tell the two apart
    assert float(((counts[free] - n / len(free)) ** 2 / (n / len(free))).sum()) > 10 * limit
    # a draw is accepted with the free rows' share of the weight
    assert attempts / n == pytest.approx(w.sum() / w[free].sum(), rel=0.02)
    # the vectorised sampler is the step-by-step one
    tab = pref.alias_table(w)
    for p in (0, 1, 599, 59999):
        assert pref.proposal_row(5, p, 0, 3, M, tab, pos)[0] == neg[p]


def test_a_context_with_one_row_left_always_gets_it():
    """M - 1 of M = 120 rows positive: every pair receives row 77; `forced` equals the scalar twin's count, pair by pair."""
    M, n = 120, 400
    pos = np.setdiff1d(np.arange(M), [77])
    tab = pref.alias_table((1.0 + np.arange(M)) ** 0.75)
    neg, attempts, forced = pref.sample(9, 2, np.zeros(n, np.int64), np.array([0, M - 1]), pos, M, tab)
    assert (neg == 77).all()
    by_hand = [pref.proposal_row(9, p, 0, 2, M, tab, pos) for p in range(n)]
    assert all(r == 77 for r, _, _ in by_hand)
    assert forced == sum(f for _, _, f in by_hand) and attempts == sum(a for _, a, _ in by_hand)
    assert 0 < forced < n and all(a == pref.MAX_ATTEMPTS for _, a, f in by_hand if f)
    # candidates are the same rule under the group offset: candidate 0 is the draw, the others differ on an open context
    rows, _, _ = pref.candidates(9, 2, np.zeros(50, np.int64), np.array([0, 3]), np.array([1, 5, 9]), M, 4, tab)
    assert np.array_equal(rows[:, 0], pref.sample(9, 2, np.zeros(50, np.int64), np.array([0, 3]), np.array([1, 5, 9]), M, tab)[0])
    assert (rows[:, 1] != rows[:, 0]).mean() > 0.8 and rows[7, 3] == pref.proposal_row(9, 7, 3, 2, M, tab, [1, 5, 9])[0]


def test_equal_weights_draw_validly_and_not_the_uniform_rules_bits():
    """Equal weights give the uniform distribution by another route — two words an attempt, 32 attempts — so the rows are valid
    draws and (documented in the header) not the uniform rule's.  Asserted: validity."""
    P = bref.make_problem(78, 8)
    ctx = np.repeat(P["ctx"], P["n_neg"])
    neg, attempts, forced = pref.draw(P, 4, pref.alias_table(np.ones(P["M"])))
    assert neg.dtype == np.int32 and ((neg >= 0) & (neg < P["M"])).all() and forced == 0 and attempts >= len(neg)
    key = set((np.repeat(np.arange(P["n_ctx"]), np.diff(P["ptr"])) * P["M"] + P["rows"]).tolist())
    assert not any(int(u) * P["M"] + int(r) in key for u, r in zip(ctx, neg))
    hdr = open(os.path.join(ROOT, "include", "fmhip_proposal.h")).read()
    assert "Equal weights give the uniform DISTRIBUTION and not the uniform rule's bits" in hdr


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------

def small_blocks():
    from sparkfm_amd import DataSet
    users = DataSet.from_rows([(0.0, ([0], [1.0])), (0.0, ([1], [1.0])), (0.0, ([], []))], batch_rows=0)
    items = DataSet.from_rows([(0.0, ([3 + j], [1.0])) for j in range(4)], batch_rows=0)
    return users, items, [[2, 0, 2], [3], [2]]


def test_python_keyword_and_refusals():
    from sparkfm_amd import HipBPR
    users, items, pos = small_blocks()
    assert HipBPR.NEGATIVES == ("uniform", "popularity")
    assert HipBPR.run(users, items, pos).proposal is None and HipBPR.run(users, items, pos, negatives="uniform").proposal is None
    b = HipBPR.run(users, items, pos, negatives="popularity")
    assert np.array_equal(b.proposal, (np.array([1.0, 0.0, 2.0, 1.0]) + 1.0) ** 0.75)       # row 2: contexts 0 and 2; the repeat counts once
    assert np.array_equal(HipBPR.run(users, items, pos, negatives="popularity", power=1.0, smooth=0.5).proposal, [1.5, 0.5, 2.5, 1.5])
    for kw in ({"n_candidates": 8}, {"sampler": "warp", "n_candidates": 8}, {"redraw": "batch"}):
        assert HipBPR.run(users, items, pos, negatives="popularity", **kw).proposal is not None
    given = HipBPR.run(users, items, pos, negatives=[1, 2, 3, 4])
    assert given.proposal.dtype == np.float64 and given.proposal.tolist() == [1.0, 2.0, 3.0, 4.0]
    for bad in (0.0, -1.0, float("nan"), True, "1", None):
        with pytest.raises(ValueError, match="smooth must be"):
            HipBPR.run(users, items, pos, negatives="popularity", smooth=bad)
    with pytest.raises(ValueError, match="power must be a finite number"):
        HipBPR.run(users, items, pos, negatives="popularity", power=float("inf"))
    with pytest.raises(ValueError, match="negatives must be one of 'uniform', 'popularity'"):
        HipBPR.run(users, items, pos, negatives="pop")
    # a refused weight vector leaves the proposal that was in force (no handle exists: no device is touched)
    before = given.proposal
    for bad, what in (([1, 0, 1, 1], r"weights\[1\] = 0.0"), ([1, 1, -2, 1], r"weights\[2\] = -2.0"), ([np.nan, 1, 1, 0], r"weights\[0\] = nan"),
                      ([1, 1, 1, np.inf], r"weights\[3\] = inf"), ([1, 1, 1], r"shape \(4,\)"), ([1, 1, 1, 1, 1], r"shape \(4,\)"),
                      ([[1, 1], [1, 1]], r"shape \(4,\)"), ([1e308] * 4, "sum of the weights is not finite"), ("uniform", "array of 4 weights")):
        with pytest.raises(ValueError, match=what):
            given.set_proposal(bad)
        assert given.proposal is before
        if not isinstance(bad, str):
            with pytest.raises(ValueError, match=what):
                HipBPR.run(users, items, pos, negatives=bad)
    given.set_proposal(None)
    assert given.proposal is None
    with pytest.raises(ValueError, match="the proposal is uniform"):
        given.proposal_table()
    given.set_proposal(np.array([4.0, 3.0, 2.0, 1.0]))
    assert given.proposal.tolist() == [4.0, 3.0, 2.0, 1.0]
    with pytest.raises(ValueError):
        given.proposal[0] = 9.0                     # (read-only: the handle holds the table of these weights)
    with pytest.raises(AttributeError):
        given.proposal = None                       # set_proposal is the way


# ---- the host arithmetic under the sanitizers ------------------------------------------------------------------------------------------

def test_table_and_draws_under_the_sanitizers(tmp_path):
    """tests/host_bpr_proposal_harness.cpp with fmhip_host.cpp under AddressSanitizer and UBSan (a program of its own; no preloading):
    the table the library builds, which the Python twin reproduces entry for entry, its refusals, and 400 draws — every fourth for a
    context with one row left — which the twin reproduces bit for bit: row, attempts and the forced flag."""
    exe = str(tmp_path / "host_bpr_proposal_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "host_bpr_proposal_harness.cpp"), os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("no sanitizer runtime for g++ in this image")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    for seed, n_ctx, M, n_inter, t in ((20261021, 12, 120, 500, 0), (5, 3, 2, 4, 7), (2 ** 40 + 3, 5, 33, 100, 4000000000)):
        r = subprocess.run([exe, str(seed), str(n_ctx), str(M), str(n_inter), "400", str(t)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env,
                           timeout=300)
        assert r.returncode == 0 and b"checks ok" in r.stdout, (seed, r.stderr.decode()[-3000:])
        lines = r.stdout.decode().splitlines()
        ptr = np.array(lines[0].split()[1:], np.int64)
        rows = np.array(lines[1].split()[1:], np.int32)
        w = np.array(lines[2].split()[1:], np.float64)
        table = np.array([[int(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("T ")], np.int64)
        draws = [tuple(int(x) for x in ln.split()[1:]) for ln in lines if ln.startswith("D ")]
        assert lines[2].startswith("W") and len(ptr) == n_ctx + 1 and len(w) == M and len(draws) == 400
        thresh, alias = pref.alias_table(w)
        assert np.array_equal(table[:, 0], np.arange(M)) and np.array_equal(table[:, 1], thresh) and np.array_equal(table[:, 2], alias)
        assert M == 2 or (alias != np.arange(M)).sum() > M // 4          # (most buckets are redirected: the heavy rows take them)
        n_forced = 0
        for p, u, c, row, attempts, forced in draws:
            assert pref.proposal_row(seed, p, c, t, M, (thresh, alias), rows[ptr[u]:ptr[u + 1]]) == (row, attempts, forced), (seed, p)
            n_forced += forced
        assert {c for _, _, c, _, _, _ in draws} == {0, 1, 2, 3, 63}
        assert (n_forced > 0) == (M > 2)          # one row of 120 / 33 left: such pairs are mostly forced; of 2, none in 32 attempts


# ---- the twin's learning ------------------------------------------------------------------------------------------------------------------

# the fp64 twin's held-out NDCG@10 on aref.hard_task(3) under negatives="popularity" (power 0.75, smooth 1), computed here on the CPU
# with the settings under which test_host_bpr_adaptive.py / test_host_warp.py pin the uniform proposal's numbers
TWIN_NDCG = {"keep": 0.1693, "best": 0.2835, "warp": 0.4515}
SETTINGS = {"keep": dict(C=1, warp=False, eta=1.0), "best": dict(C=8, warp=False, eta=1.0), "warp": dict(C=8, warp=True, eta=0.3)}


def twin_run(T, S, weights_of, seed=3):
    P = aref.task_problem(T, seed, 8, 3)
    s0 = ref.State(P["w0"], P["w"], P["v"], 0.1)
    s, _ = pref.epochs(s0.copy(), P, 30, 128, S["eta"], 0.0, 1e-3, 1e-3, ref.Rule("logistic", True, 1e-10), pref.alias_table(weights_of(P)), S["C"],
                       S["warp"], 1.0)
    return aref.twin_ndcg(T, P, s)


@pytest.mark.parametrize("name", ["keep", "best", "warp"])
def test_twin_ndcg_on_the_harder_planted_task_under_the_popularity_proposal(name):
    """The numbers the README and the GPU test quote, from the fp64 twin alone: 30 epochs, k = 8, n_neg = 3, batches of 128 pairs,
    AdaGrad.  Under the uniform proposal the same settings give 0.1004 (keep the draw), 0.3064 (best of 8) and 0.5554 (WARP at 8),
    and the popularity ranking 0.1193: the popularity proposal lifts the keep-the-draw rule above the popularity ranking and LOWERS
    both scored rules on this task.  Nothing is asserted about which proposal is better."""
    got = twin_run(aref.hard_task(3), SETTINGS[name], pref.popularity)
    print("%s under popularity^0.75: %.17g" % (name, got))
    assert got == pytest.approx(TWIN_NDCG[name], abs=5e-5), (name, got)
