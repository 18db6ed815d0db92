"""Per-row example weights, host surface (no GPU): the fp64 twin of weight_ref.py against central differences of the weighted
objective, the header against the binding, the refusal of bad weights by the C calls (before any HIP call: they run here),
DataSet's weights through from_rows / from_pairs / from_arrays / splitByRandom, and the validation pass of fmhip_host.cpp as a
stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import weight_ref as wref
from helpers import random_problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the twin is the gradient step of (1/|B|) sum c l ---------------------------------------------------------------------

@pytest.mark.parametrize("pairs", [False, True])
@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_twin_step_is_the_gradient_of_the_weighted_objective(loss, pairs):
    """One twin step with eta = 1 and no decay moves every parameter by minus the gradient of J = (1/|B|) sum_r c_r l_r (pairs:
    sum_j c_2j l_j).  Each is pinned to a central difference of J with step h = 1e-5 on a dense 8-row, 6-feature, 3-factor
    problem.  A row's yhat is LINEAR in any single parameter t (a row stores a feature once: the v^2 x^2 terms cancel), slope
    |b_r| = |x_i (q_f - v_fi x_i)| < 3 here, so J(t) = (1/|B|) sum c_r l(a_r + b_r t) has J''' = (1/|B|) sum c_r b_r^3 l''' with
    l''' = 0 (squared) or |l'''| <= 0.1 (logistic; twice that for a pair's margin): |J'''| <= 3.5 * 27 * 0.2 < 20.  The difference
    quotient is off by at most h^2/6 * 20 < 4e-10, plus rounding 2 eps J / h < 1e-10: the bound is 2e-9.
    Row 2j+1's weight differs from row 2j's in the pair cases: it must not matter."""
    a = random_problem(5, 8, 6, 3, 6, 6, scale=0.3)
    if loss == "logistic":
        a["y"] = (np.arange(8) % 3 == 0).astype(np.float64)
    c = np.array([0.25, 3.5, 0.0, 1.0, 3.5, 0.25, 1.0, 0.0])
    rule = wref.Rule(loss, pairs, None)
    rp, col, val, y = a["row_ptr"], a["col"], a["val"], a["y"]
    s0 = wref.State(a["w0"], a["w"], a["v"])
    s1 = wref.step(s0.copy(), rp, col, val, y, c, 0, 8, 1.0, 0.0, 0.0, 0.0, rule)
    J = lambda w0, w, v: wref.objective(w0, w, v, rp, col, val, y, c, 0, 8, loss, pairs)      # noqa: E731
    h, tol = 1e-5, 2e-9
    assert s0.w0 - s1.w0 == pytest.approx((J(s0.w0 + h, s0.w, s0.v) - J(s0.w0 - h, s0.w, s0.v)) / (2 * h), abs=tol)
    moved = 0.0
    for i in range(6):
        wp, wm = s0.w.copy(), s0.w.copy()
        wp[i] += h
        wm[i] -= h
        assert s0.w[i] - s1.w[i] == pytest.approx((J(s0.w0, wp, s0.v) - J(s0.w0, wm, s0.v)) / (2 * h), abs=tol), i
        for f in range(3):
            vp, vm = s0.v.copy(), s0.v.copy()
            vp[f, i] += h
            vm[f, i] -= h
            assert s0.v[f, i] - s1.v[f, i] == pytest.approx((J(s0.w0, s0.w, vp) - J(s0.w0, s0.w, vm)) / (2 * h), abs=tol), (f, i)
            moved = max(moved, abs(s0.v[f, i] - s1.v[f, i]))
    assert moved > 1e-3                       # a gradient far above the tolerance was compared
    if pairs:
        c2 = c.copy()
        c2[1::2] = [7.0, 0.5, 0.0, 9.0]       # row 2j+1's weight is not read
        s2 = wref.step(s0.copy(), rp, col, val, y, c2, 0, 8, 1.0, 0.0, 0.0, 0.0, rule)
        assert np.array_equal(s1.v, s2.v) and np.array_equal(s1.w, s2.w) and s1.w0 == s2.w0
        e = wref.weighted_residuals(np.linspace(-1, 1, 8), y, c, loss, True)
        assert np.array_equal(e[0::2], -e[1::2])


def test_twin_with_unit_weights_is_train_ref():
    import train_ref
    a = random_problem(6, 10, 7, 2, 2, 5)
    for rule in (wref.Rule("squared", False, None), wref.Rule("logistic", True, 1e-10)):
        s = wref.step(wref.State(a["w0"], a["w"], a["v"], 0.1), a["row_ptr"], a["col"], a["val"], a["y"], np.ones(10), 0, 10, 0.05, 1e-3, 1e-3, 1e-3, rule)
        t = train_ref.step(train_ref.State(a["w0"], a["w"], a["v"], 0.1), a["row_ptr"], a["col"], a["val"], a["y"], 0, 10, 0.05, 1e-3, 1e-3, 1e-3, rule)
        assert np.allclose(s.v, t.v, rtol=0, atol=1e-15) and np.allclose(s.w, t.w, rtol=0, atol=1e-15) and abs(s.w0 - t.w0) <= 1e-15


def test_reference_weighted_scores():
    s = wref.weighted_scores([0.5, -1.0, 2.0], [1.0, 0.0, 0.0], [2.0, 0.0, 0.5])
    assert s["sum_w"] == 2.5
    assert s["rmse"] == pytest.approx(np.sqrt((2.0 * 0.25 + 0.5 * 4.0) / 2.5), rel=1e-15)
    assert s["mae"] == pytest.approx((2.0 * 0.5 + 0.5 * 2.0) / 2.5, rel=1e-15)
    assert s["logloss"] == pytest.approx((2.0 * -np.log(wref.ref.sigmoid(0.5)) + 0.5 * -np.log(1 - wref.ref.sigmoid(2.0))) / 2.5, rel=1e-14)
    z = wref.weighted_scores([np.inf, 1.0], [0.0, 1.0], [0.0, 0.0])
    assert z["sum_w"] == 0.0 and all(np.isnan(z[k]) for k in ("rmse", "mae", "logloss"))


# ---- symbols ---------------------------------------------------------------------------------------------------------

def test_header_matches_the_binding():
    from sparkfm_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_weights.h")).read()
    declared = set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_WEIGHTS) == {"fmhip_dataset_create_weighted", "fmhip_rows_create_weighted", "fmhip_dataset_weights",
                                                    "fmhip_weighted_scores"}
    others = _ffi.SYMBOLS + _ffi.SYMBOLS_EXPERIMENTAL + _ffi.SYMBOLS_TOPK + _ffi.SYMBOLS_PAIRING + _ffi.SYMBOLS_METRICS + _ffi.SYMBOLS_RANKING
    assert not set(_ffi.SYMBOLS_WEIGHTS) & set(others)
    L = _ffi.load()
    for name in _ffi.SYMBOLS_WEIGHTS:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    # the result struct: the header's fields in order, 56 bytes
    m = re.search(r"typedef struct fmhip_weighted_result \{(.*?)\} fmhip_weighted_result;", hdr, re.S)
    fields = re.findall(r"^\s*(?:int32_t|int64_t|double)\s+(\w+);", m.group(1), re.M)
    assert fields == [name for name, _ in _ffi.WeightedResult._fields_]
    assert C.sizeof(_ffi.WeightedResult) == 56 and _ffi.WeightedResult().struct_size == 56
    # the public classes
    from sparkfm_amd import DataSet, FMModel
    assert all(hasattr(FMModel, n) for n in ("weightedScores", "computeWeightedRMSE", "computeWeightedLogLoss"))
    assert DataSet(np.zeros(1, np.int64), [], [], []).weights is None


def test_scores_refuse_bad_arguments_without_a_device():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    assert L.fmhip_weighted_scores(None, None, None) == -1 and b"NULL" in L.fmhip_last_error()
    res = _ffi.WeightedResult()
    res.struct_size = 8
    assert L.fmhip_weighted_scores(None, None, C.byref(res)) == -1 and b"struct_size" in L.fmhip_last_error()
    assert L.fmhip_weighted_scores(None, None, C.byref(_ffi.WeightedResult())) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_dataset_weights(None, None, None, None) == -1 and b"NULL" in L.fmhip_last_error()


# ---- bad weights: refused by the C calls, before any HIP call ------------------------------------------------------------

ROWS = dict(rp=np.array([0, 2, 3, 3, 5, 6], np.int64), col=np.array([1, 4, 2, 0, 3, 4], np.int32),
            val=np.array([1.0, 0.5, 2.0, 1.0, 1.0, 0.25]), y=np.array([1.0, 0.0, 1.0, 0.0, 1.0]))


@pytest.mark.parametrize("bad,row", [(np.nan, 3), (np.inf, 0), (-np.inf, 4), (-0.5, 2), (-1e-300, 1), (1e39, 2)])
def test_c_calls_refuse_a_bad_weight_and_name_the_row(bad, row):
    """NaN, +-inf, a negative weight, one that is not finite as fp32: FMHIP_ERR_INVALID from both weighted constructors with a
    message naming the FIRST offending row — checked on the host before the device is touched, so this runs without a GPU (an
    all-good array would go on to the device: not tried here)."""
    from sparkfm_amd import _ffi
    L = _ffi.load()
    w = np.array([1.0, 0.25, 0.0, 3.5, 1.0])
    w[row] = bad
    if row < 4:
        w[4] = -2.0                           # a later offender: the first one is named
    h = C.c_void_p(7)
    opts = _ffi.DatasetOpts(C.sizeof(_ffi.DatasetOpts), -1, 2, -1)
    args = (0, 5, _ffi.ptr(ROWS["rp"]), _ffi.ptr(ROWS["col"]), _ffi.ptr(ROWS["val"]), _ffi.ptr(ROWS["y"]), _ffi.ptr(w))
    for rc in (L.fmhip_dataset_create_weighted(*args, C.byref(opts), C.byref(h)), L.fmhip_dataset_create_weighted(*args, None, C.byref(h)),
               L.fmhip_rows_create_weighted(*args, C.byref(h))):
        assert rc == -1 and h.value is None
        msg = L.fmhip_last_error().decode()
        assert "weight[%d]" % row in msg and "finite" in msg and ">= 0" in msg, msg
    # and through the Python class: the same refusal, as FmhipError
    from sparkfm_amd import DataSet
    ds = DataSet(ROWS["rp"], ROWS["col"], ROWS["val"], ROWS["y"], weights=w, batch_rows=2)
    with pytest.raises(_ffi.FmhipError, match=r"weight\[%d\]" % row) as ei:
        ds.cache()
    assert ei.value.code == -1
    ds_s = DataSet(ROWS["rp"], ROWS["col"], ROWS["val"], ROWS["y"], weights=w, scoring=True)
    with pytest.raises(_ffi.FmhipError, match=r"weight\[%d\]" % row):
        ds_s.cache()


def test_bad_opts_and_wrong_length_are_refused():
    from sparkfm_amd import DataSet, _ffi
    L = _ffi.load()
    w = np.ones(5)
    h = C.c_void_p()
    opts = _ffi.DatasetOpts(4, -1, 2, -1)                 # a struct_size that is not the struct's
    assert L.fmhip_dataset_create_weighted(0, 5, _ffi.ptr(ROWS["rp"]), _ffi.ptr(ROWS["col"]), _ffi.ptr(ROWS["val"]), _ffi.ptr(ROWS["y"]),
                                           _ffi.ptr(w), C.byref(opts), C.byref(h)) == -1
    assert b"struct_size" in L.fmhip_last_error()
    for bad in (np.ones(4), np.ones(6), np.ones((5, 1)), 1.0):
        with pytest.raises(ValueError, match="one weight per row"):
            DataSet(ROWS["rp"], ROWS["col"], ROWS["val"], ROWS["y"], weights=bad)
    with pytest.raises(ValueError, match="one weight per row"):
        DataSet.from_rows([(1.0, ([1], [1.0])), (0.0, ([2], [1.0]))], weights=[1.0])
    with pytest.raises(ValueError, match="one weight per row"):
        DataSet.from_pairs([([1], [1.0])], [([2], [1.0])], weights=[1.0, 2.0])         # one weight per PAIR
    ok = DataSet(ROWS["rp"], ROWS["col"], ROWS["val"], ROWS["y"], weights=[1, 2, 3, 4, 5])
    assert ok.weights.dtype == np.float64 and ok.weights.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]


# ---- the Python classes carry the weights ------------------------------------------------------------------------------

def test_from_rows_from_pairs_from_arrays_carry_weights():
    from sparkfm_amd import DataSet
    rows = [(1.0, ([1, 5], [1.0, 0.5])), (0.0, ([2], [2.0])), (1.0, ([], []))]
    ds = DataSet.from_rows(rows, weights=[0.25, 0.0, 3.5])
    assert ds.weights.tolist() == [0.25, 0.0, 3.5] and DataSet.from_rows(rows).weights is None
    assert [r[0] for r in ds.rows()] == [1.0, 0.0, 1.0]                               # rows() is unchanged
    pref = [([1, 5], [1.0, 0.5]), ([2], [2.0]), ([], [])]
    oth = [([3], [0.25]), ([4, 6, 7], [1.0, 1.0, 3.0]), ([9], [1.0])]
    dp = DataSet.from_pairs(pref, oth, weights=[3.5, 0.0, 0.25], batch_rows=3)
    assert dp.size == 6 and dp.batch_rows == 4
    for j, wj in enumerate([3.5, 0.0, 0.25]):                                         # pair j's weight at rows 2j and 2j+1
        assert dp.weights[2 * j] == wj and dp.weights[2 * j + 1] == wj
    assert DataSet.from_pairs(pref, oth).weights is None
    d = dict(row_ptr=ds.row_ptr, col=ds.col, val=ds.val, y=ds.y, weights=np.array([1.0, 2.0, 3.0]))
    assert DataSet.from_arrays(d).weights.tolist() == [1.0, 2.0, 3.0]
    assert DataSet.from_arrays(d, weights=[4.0, 5.0, 6.0]).weights.tolist() == [4.0, 5.0, 6.0]      # the keyword wins
    del d["weights"]
    assert DataSet.from_arrays(d).weights is None


def test_split_by_random_carries_the_weights_of_the_rows_drawn():
    from sparkfm_amd import DataCollection, DataSet
    a = random_problem(3, 200, 30, 2, 1, 5)
    w = np.arange(200, dtype=np.float64) + 0.5              # a weight that names its row
    a["y"] = np.arange(200, dtype=np.float64)               # ... and a label that does too
    raw = DataSet(a["row_ptr"], a["col"], a["val"], a["y"], weights=w)
    dc = DataCollection.splitByRandom(raw, 0.6, 0.2, 0.2, seed=4)
    parts = (dc.trainingSet, dc.testSet, dc.validationSet)
    assert sum(p.size for p in parts) == 200 and all(p.size > 10 for p in parts)
    for p in parts:
        assert p.weights is not None and np.array_equal(p.weights, p.y + 0.5)
    assert dc.testSet.scoring and dc.validationSet.scoring and not dc.trainingSet.scoring
    plain = DataCollection.splitByRandom(DataSet(a["row_ptr"], a["col"], a["val"], a["y"]), 0.6, 0.2, 0.2, seed=4)
    assert all(p.weights is None for p in (plain.trainingSet, plain.testSet, plain.validationSet))
    assert np.array_equal(plain.trainingSet.y, dc.trainingSet.y)              # the same rows are drawn with and without weights


# ---- the validation pass under the sanitizers ---------------------------------------------------------------------------

def test_weight_validation_under_the_sanitizers(tmp_path):
    """tests/host_weights_harness.cpp with fmhip_host.cpp under AddressSanitizer and UBSan: a program of its own over seeded
    weight arrays (exactly n doubles each), offenders planted at seeded rows, 1 .. 7 threads."""
    exe = str(tmp_path / "host_weights_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "host_weights_harness.cpp"), os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("no sanitizer runtime for g++ in this image")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    for seed in (20261019, 5):
        r = subprocess.run([exe, str(seed), "150"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
        assert r.returncode == 0 and b"checks ok" in r.stdout, (seed, r.stderr.decode()[-3000:])
