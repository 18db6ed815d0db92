"""Adaptive negatives of the BPR trainer, host surface (no GPU): the header against the binding and the exported symbols, the refusals
that need no device, the fp64 twin (bpr_adaptive_ref.py) against bpr_ref's uniform sampler and against a step-by-step restatement,
the first-strict-maximum choice, and the host twin of fmhip_host.cpp (bpr_candidate) as a stand-alone program under AddressSanitizer
and UBSan that recomputes vectors recorded from the Python twin."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bpr_adaptive_ref as aref
import bpr_ref as bref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- symbols -------------------------------------------------------------------------------------------------------------------------

def declared_in(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))


def test_header_matches_the_binding_and_the_library():
    from sparkfm_amd import _build, _ffi
    names = {"fmhip_bpr_set_candidates", "fmhip_bpr_get_candidates", "fmhip_bpr_resample_adaptive"}
    assert declared_in("fmhip_bpr_adaptive.h") == set(_ffi.SYMBOLS_BPR_ADAPTIVE) == names
    others = (_ffi.SYMBOLS + _ffi.SYMBOLS_EXPERIMENTAL + _ffi.SYMBOLS_TOPK + _ffi.SYMBOLS_PAIRING + _ffi.SYMBOLS_METRICS + _ffi.SYMBOLS_RANKING
              + _ffi.SYMBOLS_WEIGHTS + _ffi.SYMBOLS_RELATIONAL + _ffi.SYMBOLS_MCMC + _ffi.SYMBOLS_MCMC_TASK + _ffi.SYMBOLS_MCMC_GROUPS
              + _ffi.SYMBOLS_MCMC_RELATIONAL + _ffi.SYMBOLS_BPR)
    assert not names & set(others)
    # fmhip_bpr.h and its list are what they were
    assert declared_in("fmhip_bpr.h") == set(_ffi.SYMBOLS_BPR) == {"fmhip_bpr_" + n for n in ("create", "destroy", "info", "resample", "negatives",
                                                                                              "step", "epoch", "pair_logloss")}
    assert "adaptive" not in open(os.path.join(ROOT, "include", "fmhip_bpr.h")).read()
    assert "fmhip_bpr_debug_adaptive" in _ffi.SYMBOLS_EXPERIMENTAL and "fmhip_bpr_debug_adaptive" in declared_in("fmhip_experimental.h")
    L = _ffi.load()
    for name in _ffi.SYMBOLS_BPR_ADAPTIVE + ("fmhip_bpr_debug_adaptive",):
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int, name
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], stdout=subprocess.PIPE, check=True).stdout.decode()
    exported = set(re.findall(r"\bT (fmhip_bpr_[a-z0-9_]+)", out))
    assert exported == set(_ffi.SYMBOLS_BPR) | names | {"fmhip_bpr_debug_inverse", "fmhip_bpr_debug_adaptive"}
    assert os.path.join("..", "..", "include", "fmhip_bpr_adaptive.h") in _build.HIP_DEPS
    hdr = open(os.path.join(ROOT, "include", "fmhip_bpr_adaptive.h")).read()
    assert re.search(r"#define FMHIP_BPR_MAX_CANDIDATES (\d+)", hdr).group(1) == str(_ffi.BPR_MAX_CANDIDATES) == str(aref.MAX_CANDIDATES) == "64"
    assert [n for n, _ in _ffi.BprAdaptiveStats._fields_] == re.findall(r"int64_t (\w+);", hdr) == ["attempts", "forced", "replaced"]
    # the sampler's shared integer code takes the group offset; nothing else draws negatives
    rng_h = open(os.path.join(ROOT, "sparkfm_amd", "csrc", "mcmc_rng.h")).read()
    assert "uint32_t group0 = 0" in rng_h and rng_h.count("t, kStreamNegative);") == 1


def test_c_calls_refuse_null_handles_and_bad_counts_without_a_device():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    n = C.c_int32(-5)
    st = _ffi.BprAdaptiveStats()
    assert L.fmhip_bpr_set_candidates(None, 4) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error()
    assert L.fmhip_bpr_get_candidates(None, C.byref(n)) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error() and n.value == -5
    assert L.fmhip_bpr_resample_adaptive(None, None, 0, C.byref(st)) == -1 and b"NULL" in L.fmhip_last_error()
    i, f = np.zeros(1, np.int32), np.zeros(1, np.float32)
    assert L.fmhip_bpr_debug_adaptive(None, None, 0, 0, 1, _ffi.ptr(i), _ffi.ptr(f)) == -1 and b"NULL" in L.fmhip_last_error()


def test_python_validates_n_candidates_at_construction():
    from sparkfm_amd import DataSet, HipBPR
    users = DataSet.from_rows([(0.0, ([0], [1.0])), (0.0, ([1], [1.0])), (0.0, ([], []))], batch_rows=0)
    items = DataSet.from_rows([(0.0, ([3 + j], [1.0])) for j in range(4)], batch_rows=0)
    pos = [[2, 0, 2], [3], []]
    assert HipBPR.run(users, items, pos).n_candidates == 1
    assert HipBPR.run(users, items, pos, n_candidates=64).n_candidates == 64
    assert HipBPR.run(users, items, pos, n_candidates=np.int64(5)).n_candidates == 5
    for bad in (0, 65, -1):
        with pytest.raises(ValueError, match=r"n_candidates must be in \[1, 64\], not %d" % bad):
            HipBPR.run(users, items, pos, n_candidates=bad)
    for bad in (2.5, "4", None, True):
        with pytest.raises(TypeError):
            HipBPR.run(users, items, pos, n_candidates=bad)
    with pytest.raises(AttributeError):
        HipBPR.run(users, items, pos).n_candidates = 3          # fixed at construction
    # no model, several candidates: refused before any device call
    with pytest.raises(ValueError, match="needs a model"):
        HipBPR.run(users, items, pos, n_candidates=2).resample(0)


# ---- the twin ------------------------------------------------------------------------------------------------------------------------

def test_twin_candidate_0_is_the_uniform_sampler():
    P = bref.make_problem(11, 4, n_neg=3)
    ctx = np.repeat(P["ctx"], 3)
    for t in (0, 7):
        rows, attempts, forced = aref.candidates(P["seed"], t, ctx, P["ptr"], P["rows"], P["M"], 5)
        neg, a1, f1 = bref.draw(P, t)
        assert rows.dtype == np.int32 and rows.shape == (1800, 5) and np.array_equal(rows[:, 0], neg)
        one = aref.candidates(P["seed"], t, ctx, P["ptr"], P["rows"], P["M"], 1)
        assert np.array_equal(one[0][:, 0], neg) and one[1:] == (a1, f1)
        assert attempts >= 5 * 1800 and forced == 0
        # the candidates are independent draws: columns differ from one another, and none is a positive
        key = set((np.repeat(np.arange(P["n_ctx"]), np.diff(P["ptr"])) * P["M"] + P["rows"]).tolist())
        for c in range(1, 5):
            assert (rows[:, c] != rows[:, 0]).mean() > 0.9
            assert not any(int(u) * P["M"] + int(r) in key for u, r in zip(ctx, rows[:, c]))
        # the vectorised twin is the step-by-step one, and that one's c = 0 is bpr_ref.negative
        for p in (0, 1, 599, 1799):
            lst = P["rows"][P["ptr"][ctx[p]]:P["ptr"][ctx[p] + 1]]
            assert aref.candidate(P["seed"], p, 0, t, P["M"], lst) == bref.negative(P["seed"], p, t, P["M"], lst)
            for c in (1, 4):
                assert aref.candidate(P["seed"], p, c, t, P["M"], lst)[0] == rows[p, c]


def test_twin_forced_context_and_two_rows():
    """119 of 120 rows positive: every candidate is row 77, forced or not; M = 2 with one positive: always the other row."""
    M = 120
    pos = np.setdiff1d(np.arange(M), [77])
    rows, attempts, forced = aref.candidates(9, 2, np.zeros(50, np.int64), np.array([0, M - 1]), pos, M, 64)
    assert (rows == 77).all() and 0.45 * 3200 < forced < 0.72 * 3200          # (119/120)^64 = 0.585 of the candidates
    by_hand = [aref.candidate(9, p, c, 2, M, pos) for p in range(3) for c in (0, 1, 63)]
    assert all(r == 77 for r, _, _ in by_hand)
    rows2, attempts2, forced2 = aref.candidates(9, 2, np.arange(40) % 2, np.array([0, 1, 2]), np.array([0, 1]), 2, 5)
    assert np.array_equal(rows2, np.repeat((1 - np.arange(40) % 2)[:, None], 5, axis=1)) and forced2 == 0      # 2^-64 a candidate


def test_first_strict_maximum():
    nan = np.nan
    s = np.array([[1.0, 2.0, 2.0, 3.0, 3.0],      # the first of the 3s
                  [5.0, 5.0, 5.0, 5.0, 5.0],      # ties keep candidate 0
                  [1.0, nan, 0.5, 1.5, nan],      # a NaN never replaces
                  [nan, 9.0, 9.0, 9.0, 9.0],      # ... and a NaN incumbent is never replaced
                  [-np.inf, -np.inf, -1.0, -2.0, -1.0],
                  [0.0, -0.0, 0.0, -0.0, 0.0]])   # -0 == 0
    assert aref.first_strict_max(s).tolist() == [3, 0, 3, 0, 2, 0]
    assert aref.first_strict_max(s[:, :1]).tolist() == [0] * 6


def test_twin_ndcg_on_the_planted_tasks():
    """The numbers the GPU tests' docstrings and the README quote, from the fp64 twin alone (AdaGrad eta 1.0, regw = regv = 1e-3,
    k = 8, n_neg = 3, batches of 128 pairs, v ~ N(0, 0.05)): held-out NDCG@10 on bpr_ref.planted_task(3) after 60 epochs at
    n_candidates = 8 — 0.6308, where the uniform twin of test_gpu_bpr.py reaches 0.6447: the easy task gains nothing from hard
    negatives — and on hard_task(3) after 30 epochs: uniform 0.1004, below the popularity ranking's 0.1193, best of 8: 0.3064."""
    import train_ref as ref
    rule = ref.Rule("logistic", True, 1e-10)

    def run(T, epochs, C):
        P = aref.task_problem(T, 3, 8, 3)
        s0 = ref.State(P["w0"], P["w"], P["v"], 0.1)
        pop = np.bincount(np.concatenate(T["train"]), minlength=P["M"]).astype(np.float64)
        popular = bref.ndcg_at(np.tile(pop, (P["n_ctx"], 1)), T["held_out"], T["train"])
        s, _ = aref.epochs(s0.copy(), P, epochs, 128, 1.0, 0.0, 1e-3, 1e-3, rule, C)
        return aref.twin_ndcg(T, P, s0), popular, aref.twin_ndcg(T, P, s)

    easy = run(bref.planted_task(3), 60, 8)
    assert easy == pytest.approx((0.0921, 0.1994, 0.6308), abs=5e-5)
    T = aref.hard_task(3)
    assert [len(x) for x in T["train"]] == [15] * 60 and [len(x) for x in T["held_out"]] == [5] * 60
    uniform, hard = run(T, 30, 1), run(T, 30, 8)
    assert uniform == pytest.approx((0.0326, 0.1193, 0.1004), abs=5e-5) and hard == pytest.approx((0.0326, 0.1193, 0.3064), abs=5e-5)
    assert hard[2] > hard[1] > uniform[2] > uniform[0]


# ---- the host twin under the sanitizers ------------------------------------------------------------------------------------------------

def vectors(path):
    """Contexts and (p, c) picks recorded from the Python twin: a base list, a context with one row left, M = 2, an empty list under
    a 64-bit seed and a t past 2^31.  -> the number of V records."""
    rng = np.random.default_rng(5)
    lines, n = [], 0
    cases = [(20261020, 7, 120, np.sort(rng.choice(120, 15, replace=False)), range(0, 40), (0, 1, 5, 63)),
             (9, 2, 120, np.setdiff1d(np.arange(120), [77]), range(0, 12), (0, 3, 63)),
             (5, 0, 2, np.array([1]), range(0, 30), (0, 1, 2, 63)),
             (5, 0, 2, np.array([0]), (7, 2 ** 31 + 5), (0, 62)),
             (2 ** 40 + 3, 4000000000, 33, np.zeros(0, np.int64), (0, 2 ** 32 - 1), (0, 17))]
    forced = 0
    for seed, t, M, lst, ps, cs in cases:
        lines.append("L %d %d %d %d %s" % (seed, t, M, len(lst), " ".join(str(int(x)) for x in lst)))
        for p in ps:
            for c in cs:
                row, attempts, f = aref.candidate(seed, p, c, t, M, lst)
                lines.append("V %d %d %d %d %d" % (p, c, row, attempts, f))
                n += 1
                forced += f
    assert forced > 5          # the forced walk is in the record
    open(path, "w").write("\n".join(lines) + "\n")
    return n, lines


def test_host_twin_under_the_sanitizers(tmp_path):
    """tests/host_bpr_adaptive_harness.cpp with fmhip_host.cpp under AddressSanitizer and UBSan (a program of its own; no preloading)
    recomputes every recorded candidate — row, attempts and the forced flag — bit for bit; a record with one number changed fails."""
    exe = str(tmp_path / "host_bpr_adaptive_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "host_bpr_adaptive_harness.cpp"), os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("no sanitizer runtime for g++ in this image")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    path = str(tmp_path / "vectors.txt")
    n, lines = vectors(path)
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert r.returncode == 0 and ("checks ok %d" % n).encode() in r.stdout, r.stderr.decode()[-3000:]
    # the program does compare: the first record's row moved by one
    v = lines[1].split()
    lines[1] = " ".join(v[:3] + [str((int(v[3]) + 1) % 120)] + v[4:])
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("\n".join(lines) + "\n")
    r = subprocess.run([exe, bad], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert r.returncode == 1 and b"check failed" in r.stderr and b"checks ok" not in r.stdout
