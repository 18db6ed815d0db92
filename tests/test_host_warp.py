"""WARP for the BPR trainer, host surface (no GPU): the header against the binding and the exported symbols, the refusals that need no
device, the Python keywords, the weight table against exact rational sums, the first-violator rule on a hand table, the fp64 twin's
(warp_ref.py) NDCG on the planted tasks, and the host twin of fmhip_host.cpp (warp_weight_table, warp_first_violator) as a stand-alone
program under AddressSanitizer and UBSan that recomputes vectors recorded from the Python twin."""
import ctypes as C
import os
import re
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import bpr_adaptive_ref as aref
import bpr_ref as bref
import warp_ref as wref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARP_NAMES = {"fmhip_warp_" + n for n in ("set", "get", "resample", "weights", "trials")}


def declared_in(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))


# ---- symbols -------------------------------------------------------------------------------------------------------------------------

def test_header_matches_the_binding_and_the_library():
    from sparkfm_amd import _build, _ffi
    assert declared_in("fmhip_warp.h") == set(_ffi.SYMBOLS_WARP) == WARP_NAMES
    others = (_ffi.SYMBOLS + _ffi.SYMBOLS_EXPERIMENTAL + _ffi.SYMBOLS_TOPK + _ffi.SYMBOLS_PAIRING + _ffi.SYMBOLS_METRICS + _ffi.SYMBOLS_RANKING
              + _ffi.SYMBOLS_WEIGHTS + _ffi.SYMBOLS_RELATIONAL + _ffi.SYMBOLS_MCMC + _ffi.SYMBOLS_MCMC_TASK + _ffi.SYMBOLS_MCMC_GROUPS
              + _ffi.SYMBOLS_MCMC_RELATIONAL + _ffi.SYMBOLS_BPR + _ffi.SYMBOLS_BPR_ADAPTIVE)
    assert not WARP_NAMES & set(others)
    assert "fmhip_warp_debug" in _ffi.SYMBOLS_EXPERIMENTAL and "fmhip_warp_debug" in declared_in("fmhip_experimental.h")
    L = _ffi.load()
    for name in _ffi.SYMBOLS_WARP + ("fmhip_warp_debug",):
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int, name
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert set(re.findall(r"\bT (fmhip_warp_[a-z0-9_]+)", out)) == WARP_NAMES | {"fmhip_warp_debug"}
    # the fmhip_bpr_* set is what it was: nothing of WARP is exported under that prefix
    assert set(re.findall(r"\bT (fmhip_bpr_[a-z0-9_]+)", out)) == set(_ffi.SYMBOLS_BPR) | set(_ffi.SYMBOLS_BPR_ADAPTIVE) | {
        "fmhip_bpr_debug_inverse", "fmhip_bpr_debug_adaptive"}
    assert "warp" not in open(os.path.join(ROOT, "include", "fmhip_bpr.h")).read().lower()
    assert "warp" not in open(os.path.join(ROOT, "include", "fmhip_bpr_adaptive.h")).read().lower()
    assert os.path.join("..", "..", "include", "fmhip_warp.h") in _build.HIP_DEPS
    hdr = open(os.path.join(ROOT, "include", "fmhip_warp.h")).read()
    assert [n for n, _ in _ffi.WarpStats._fields_] == re.findall(r"int64_t (\w+);", hdr) == ["pairs", "violated", "trials"]
    # WARP draws nothing of its own: the sampler's one site
    rng_h = open(os.path.join(ROOT, "sparkfm_amd", "csrc", "mcmc_rng.h")).read()
    assert rng_h.count("t, kStreamNegative);") == 1
    # the model's losses do not learn the hinge
    with pytest.raises(ValueError):
        _ffi.loss_code("hinge")


def test_c_calls_refuse_null_handles_without_a_device():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    en, mg = C.c_int(-5), C.c_double(-5.0)
    st = _ffi.WarpStats()
    one = np.zeros(1, np.float32)
    onei = np.zeros(1, np.int32)
    assert L.fmhip_warp_set(None, 1, 1.0) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error()
    assert L.fmhip_warp_get(None, C.byref(en), C.byref(mg)) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error()
    assert (en.value, mg.value) == (-5, -5.0)
    assert L.fmhip_warp_resample(None, None, 0, C.byref(st)) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_warp_weights(None, _ffi.ptr(one)) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error()
    assert L.fmhip_warp_trials(None, _ffi.ptr(onei)) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error()
    assert L.fmhip_warp_debug(None, None, 0, 0, 1, _ffi.ptr(onei), _ffi.ptr(one), _ffi.ptr(one)) == -1 and b"NULL" in L.fmhip_last_error()


def small_blocks():
    from sparkfm_amd import DataSet
    users = DataSet.from_rows([(0.0, ([0], [1.0])), (0.0, ([1], [1.0])), (0.0, ([], []))], batch_rows=0)
    items = DataSet.from_rows([(0.0, ([3 + j], [1.0])) for j in range(4)], batch_rows=0)
    return users, items, [[2, 0, 2], [3], []]


def test_python_validates_the_keywords_at_construction():
    from sparkfm_amd import HipBPR
    users, items, pos = small_blocks()
    auto = HipBPR.run(users, items, pos)
    assert (auto.sampler, auto.warp, auto.n_candidates) == ("auto", False, 1)
    w = HipBPR.run(users, items, pos, sampler="warp", n_candidates=8)
    assert (w.sampler, w.warp, w.margin, w.n_candidates) == ("warp", True, 1.0, 8)
    assert HipBPR.run(users, items, pos, sampler="warp", margin=0).margin == 0.0
    assert HipBPR.run(users, items, pos, sampler="warp", margin=np.float32(0.25)).margin == 0.25
    for bad in ("uniform", "adaptive", "WARP", None, 1):
        with pytest.raises(ValueError, match="sampler must be one of 'auto', 'warp'"):
            HipBPR.run(users, items, pos, sampler=bad)
    for bad in (-1.0, -1e-9, float("nan"), float("inf"), 1e300, "1", None, True):
        with pytest.raises(ValueError, match="margin must be a finite number >= 0"):
            HipBPR.run(users, items, pos, sampler="warp", margin=bad)
    with pytest.raises(ValueError, match="leave loss at its default"):
        HipBPR.run(users, items, pos, sampler="warp", loss="squared")
    for loss in ("hinge", "warp"):          # the model's losses stay squared and logistic, under either sampler
        for kw in ({}, {"sampler": "warp"}):
            with pytest.raises(ValueError):
                HipBPR.run(users, items, pos, loss=loss, **kw)
    with pytest.raises(AttributeError):
        w.sampler = "auto"                   # fixed at construction
    with pytest.raises(AttributeError):
        w.margin = 2.0
    # refused before any device call: a WARP draw without a model, the adaptive record in WARP mode, WARP's reads in auto mode
    with pytest.raises(ValueError, match="needs a model"):
        w.resample(0)
    with pytest.raises(ValueError, match="use warp_draws"):
        w.candidate_draws(None, 0)
    for name in ("pair_weights", "trials"):
        with pytest.raises(ValueError, match="belongs to sampler='warp'"):
            getattr(auto, name)()
    with pytest.raises(ValueError, match="belongs to sampler='warp'"):
        auto.warp_draws(None, 0)


# ---- the weight table ----------------------------------------------------------------------------------------------------------------

def segment(a, b):
    """sum_{j = a + 1 .. b} 1 / j as a Fraction, by halves (the large denominators meet only near the top)."""
    if b - a <= 8:
        return sum((Fraction(1, j) for j in range(a + 1, b + 1)), Fraction(0))
    mid = (a + b) // 2
    return segment(a, mid) + segment(mid, b)


@pytest.mark.parametrize("M", [2, 3, 120, 100000])
def test_weight_table_against_exact_sums(M):
    """W[n] = float32(H(max(1, (M - 1) // n))) for C = 64 against H as an exact fractions.Fraction, rounded once to fp64 and then to
    fp32.  The twin sums in fp64 with j ascending: its error against the exact sum is below r * 2^-53 * H(r) < 2e-10 for r < 10^5,
    far inside half an fp32 ulp of H >= 1 (6e-8) unless the exact value sits that close to a rounding boundary — which the test
    checks it does not."""
    C_ = 64
    W = wref.weight_table(M, C_)
    assert W.dtype == np.float32 and W.shape == (C_ + 1,) and W[0] == 0.0
    exact, h, at = {}, Fraction(0), 0
    for r in sorted({max(1, (M - 1) // n) for n in range(1, C_ + 1)}):
        h, at = h + segment(at, r), r
        exact[r] = h
    for n in range(1, C_ + 1):
        r = max(1, (M - 1) // n)
        want = np.float32(float(exact[r]))
        assert W[n] == want, (M, n, r)
        for other in (np.nextafter(want, np.float32(0)), np.nextafter(want, np.float32(np.inf))):
            boundary = (Fraction(float(other)) + Fraction(float(want))) / 2
            assert abs(exact[r] - boundary) > Fraction(1, 10 ** 9), (M, n, r)
    assert (np.diff(W[1:]) <= 0).all()
    if M == 2:
        assert (W[1:] == 1.0).all()           # one negative row: rank 1, whatever the trials
    if M == 120:
        assert W[1] == np.float32(float(sum(Fraction(1, j) for j in range(1, 120)))) and W[64] == 1.0 and W[60] == 1.0 and W[59] == 1.5


# ---- the first violator ----------------------------------------------------------------------------------------------------------------

def f(*x):
    return np.array(x, np.float32)


def hand_cases():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    return [  # scores, s+, margin, N
        (f(0.0, 0.5, 1.0, 2.0), 1.5, 1.0, 3),           # thr = 0.5: the tie at candidate 1 is no violation, 1.0 is
        (f(0.5, 0.5, 0.5, 0.5), 1.5, 1.0, 0),           # all ties
        (f(nan, 0.6, 0.7, 0.1), 1.5, 1.0, 2),           # a NaN candidate never violates
        (f(9.0, 9.0, 9.0, 9.0), nan, 1.0, 0),           # a NaN positive: nothing violates
        (f(-inf, inf, 0.0, 0.0), 1.5, 1.0, 2),          # +inf violates any finite threshold
        (f(inf, inf, inf, inf), inf, 1.0, 0),           # ... and ties with an infinite one
        (f(-inf, -inf, -inf, -1e30), -inf, 1.0, 4),     # thr = -inf: -inf ties, any finite score violates
        (f(-0.0, 0.0, -0.0, 1e-45), 1.0, 1.0, 4),       # thr = 0: -0 and 0 tie with it, the smallest denormal violates
        (f(0.0, 0.0, 0.0, 0.0), 1.0, 1.0, 0),
        (f(-1.0, -2.0, -3.0, -4.0), 5.0, 1.0, 0),       # no violator
        (f(3.0, 9.0, 9.0, 9.0), 5.0, 1.0, 2),           # the lowest index, not the largest score
        (f(0.25, 0.5, 0.75, 1.0), 0.5, 0.0, 3),         # margin 0: strictly above the positive
        (f(1.0,), 1.5, 1.0, 1), (f(0.5,), 1.5, 1.0, 0), (f(nan,), 1.5, 1.0, 0)]      # C = 1


def test_first_violator_on_a_hand_table():
    for sc, sp, m, want in hand_cases():
        assert wref.first_violator(sc[None, :], f(sp), m).tolist() == [want], (sc, sp, m)
    # one subtraction in the scores' own dtype: 1 - 2^-30 is 1.0 in fp32 (a tie with the score 1.0) and below 1 in fp64 (a violation)
    assert wref.first_violator(f(1.0)[None, :], f(1.0), 2.0 ** -30).tolist() == [0]
    assert wref.first_violator(np.array([[1.0]]), np.array([1.0]), 2.0 ** -30).tolist() == [1]
    # rows and weights from N
    rows = np.array([[7, 8, 9], [4, 5, 6]], np.int32)
    neg, cw = wref.choose(rows, np.array([3, 0], np.int32), wref.weight_table(120, 3))
    assert neg.tolist() == [9, 4] and cw.tolist() == [wref.weight_table(120, 3)[3], 0.0]


# ---- the twin's learning ------------------------------------------------------------------------------------------------------------------

SETTINGS = dict(k=8, n_neg=3, batch_pairs=128, eta=0.3, regw=1e-3, regv=1e-3, epochs=30, margin=1.0)


def twin_run(T, C_, seed=3):
    import train_ref as ref
    P = aref.task_problem(T, seed, SETTINGS["k"], SETTINGS["n_neg"])
    s0 = ref.State(P["w0"], P["w"], P["v"], 0.1)
    s, _ = wref.epochs(s0.copy(), P, SETTINGS["epochs"], SETTINGS["batch_pairs"], SETTINGS["eta"], 0.0, SETTINGS["regw"], SETTINGS["regv"],
                       ref.Rule("logistic", True, 1e-10), C_, SETTINGS["margin"])
    return aref.twin_ndcg(T, P, s0), aref.twin_ndcg(T, P, s)


def test_twin_ndcg_on_the_planted_tasks():
    """The numbers the README and the GPU test quote, from the fp64 twin alone: k = 8, n_neg = 3, batches of 128 pairs, AdaGrad
    (eps 1e-10, initial accumulator 0.1) with eta = 0.3, regw = regv = 1e-3, 30 epochs, margin 1, v ~ N(0, 0.05).  Held-out NDCG@10
    on aref.hard_task(3): WARP at C = 8 0.5554, at C = 1 0.5195 — against 0.3064 for the best of 8 under the logistic loss, 0.1004
    for uniform BPR and 0.1193 for the popularity ranking (test_host_bpr_adaptive.py pins those three); on bref.planted_task(3):
    WARP at C = 8 0.6067 from 0.0921 untrained."""
    T = aref.hard_task(3)
    pop = np.bincount(np.concatenate(T["train"]), minlength=400).astype(np.float64)
    popular = bref.ndcg_at(np.tile(pop, (60, 1)), T["held_out"], T["train"])
    hard8, hard1 = twin_run(T, 8), twin_run(T, 1)
    assert popular == pytest.approx(0.1193, abs=5e-5)
    assert hard8 == pytest.approx((0.0326, 0.5554), abs=5e-5) and hard1 == pytest.approx((0.0326, 0.5195), abs=5e-5)
    assert hard8[1] > 0.3064 > popular and hard8[1] > hard1[1] > popular
    assert twin_run(bref.planted_task(3), 8) == pytest.approx((0.0921, 0.6067), abs=5e-5)


# ---- the host twin under the sanitizers ------------------------------------------------------------------------------------------------

def hx(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(x)))[0]


def vectors(path):
    """Weight tables and first-violator records from the Python twin -> (the number of records, the lines)."""
    lines = []
    for M, C_ in [(2, 64), (3, 64), (120, 64), (100000, 64), (120, 1), (65, 64), (400, 8)]:
        lines.append("W %d %d %s" % (M, C_, " ".join(hx(x) for x in wref.weight_table(M, C_))))
    for sc, sp, m, want in hand_cases():
        lines.append("F %d %s %s %d %s" % (len(sc), hx(m), hx(sp), want, " ".join(hx(x) for x in sc)))
    rng = np.random.default_rng(17)
    for C_ in (1, 5, 64):
        sc = rng.normal(0, 1, (40, C_)).astype(np.float32)
        sc[rng.random(sc.shape) < 0.05] = np.nan
        sp = rng.normal(1.0, 1, 40).astype(np.float32)
        sc[::7, -1] = sp[::7] - np.float32(0.5)          # ties at the threshold
        for m in (0.0, 0.5, 3.0):
            for s, p, n in zip(sc, sp, wref.first_violator(sc, sp, m)):
                lines.append("F %d %s %s %d %s" % (C_, hx(m), hx(p), n, " ".join(hx(x) for x in s)))
    open(path, "w").write("\n".join(lines) + "\n")
    return len(lines), lines


def test_host_twin_under_the_sanitizers(tmp_path):
    """tests/host_warp_harness.cpp with fmhip_host.cpp under AddressSanitizer and UBSan (a program of its own; no preloading)
    recomputes every recorded weight table and first violator bit for bit; a record with one number changed fails."""
    exe = str(tmp_path / "host_warp_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "host_warp_harness.cpp"), os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("no sanitizer runtime for g++ in this image")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    path = str(tmp_path / "vectors.txt")
    n, lines = vectors(path)
    assert n > 300
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert r.returncode == 0 and ("checks ok %d" % n).encode() in r.stdout, r.stderr.decode()[-3000:]
    # the program does compare: one weight of the first table moved by an ulp, then one trial count moved by one
    for at, change in ((0, lambda v: v[:4] + ["%08x" % (int(v[4], 16) + 1)] + v[5:]),
                       (7, lambda v: v[:4] + [str((int(v[4]) + 1) % (int(v[1]) + 1))] + v[5:])):
        bad_lines = list(lines)
        bad_lines[at] = " ".join(change(lines[at].split()))
        assert bad_lines[at] != lines[at]
        bad = str(tmp_path / ("bad%d.txt" % at))
        open(bad, "w").write("\n".join(bad_lines) + "\n")
        r = subprocess.run([exe, bad], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
        assert r.returncode == 1 and b"check failed" in r.stderr and b"checks ok" not in r.stdout
