"""Relational data, host surface (no GPU): the fp64 twin by block caches (relational_ref.py) against train_ref.step on the flat
expansion, expand() against a hand-written case, the header against the binding, the refusals that need no device (NULL arguments
through the C call; a mapping out of range and a shared feature through the Python constructor — the C call's own checks of those
need block handles, which need a device: test_gpu_relational.py), withRelation, and the host arithmetic of fmhip_host.cpp — mapping
check, disjointness, the inverse map's counting sort — as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import relational_ref as rref
import train_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the twin by block caches is the flat step ------------------------------------------------------------------------

@pytest.mark.parametrize("plain", [True, False])
@pytest.mark.parametrize("eps", [None, 1e-10])
@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_twin_by_block_caches_is_the_flat_step(loss, eps, plain):
    """Predictions, and one step of rows [50, 350) (SGD and AdaGrad, both losses, with and without a plain part), by block caches
    against oracle.predict / train_ref.step on the flat expansion: 1e-12 (fp64 rounding of sums of a few dozen terms of size <= 1)."""
    p = rref.base_problem(11, 5, loss, plain=plain)
    a = rref.flat(p)
    rule = train_ref.Rule(loss, False, eps)
    s0 = train_ref.State(p["w0"], p["w"], p["v"], 0.1)
    import oracle
    assert np.abs(rref.predict(s0, p) - oracle.predict(s0.w0, s0.w, s0.v, a["row_ptr"], a["col"], a["val"])).max() <= 1e-12
    s1 = rref.step(s0.copy(), p, 50, 350, 0.05, 1e-3, 2e-3, 3e-3, rule)
    t1 = train_ref.step(s0.copy(), a["row_ptr"], a["col"], a["val"], a["y"], 50, 350, 0.05, 1e-3, 2e-3, 3e-3, rule)
    assert np.abs(s1.v - t1.v).max() <= 1e-12 and np.abs(s1.w - t1.w).max() <= 1e-12 and abs(s1.w0 - t1.w0) <= 1e-12
    assert np.abs(s1.v - s0.v).max() > 1e-4                    # it moved
    # the base problem is what the issue asks for
    mi = p["maps"][1]
    assert (mi == 3).sum() == 150 and not np.isin(np.arange(80, 90), mi).any() and not np.isin(np.arange(30, 37), p["maps"][0]).any()
    assert p["blocks"][1]["row_ptr"][6] == p["blocks"][1]["row_ptr"][5] and (mi == 5).any()


# ---- expand() ----------------------------------------------------------------------------------------------------------

def test_expand_against_a_hand_written_case():
    from sparkfm_amd import DataSet, Features, Relation, RelationalData
    users = Relation([([1], [1.0]), ([2, 3], [0.5, 2.0])], [0, 1, 1, 0, 1])                                  # rows of (indices, values)
    items = Relation((np.array([0, 1, 1, 3]), np.array([5, 6, 7], np.int32), np.array([1.0, 2.0, 3.0])), [2, 2, 0, 1, 2])     # CSR; row 1 empty
    plain = DataSet.from_rows([(9.0, ([9], [1.0])), (9.0, ([], [])), (9.0, ([10, 11], [1.0, 1.0])), (9.0, ([], [])), (9.0, ([9], [2.0]))])
    rd = RelationalData([1, 2, 3, 4, 5], [users, items], plain=plain, batch_rows=2, name="r")
    assert (rd.size, rd.dimension, rd.n_batches, rd.batch_rows) == (5, 11, 3, 2)
    f = rd.expand()
    assert isinstance(f, DataSet) and f.batch_rows == 2
    assert f.row_ptr.tolist() == [0, 4, 8, 13, 14, 19]
    assert f.col.tolist() == [1, 6, 7, 9, 2, 3, 6, 7, 2, 3, 5, 10, 11, 1, 2, 3, 6, 7, 9]
    assert f.val.tolist() == [1, 2, 3, 1, 0.5, 2, 2, 3, 0.5, 2, 1, 1, 1, 1, 0.5, 2, 2, 3, 2]
    assert f.y.tolist() == [1, 2, 3, 4, 5]                      # the relational labels, not the plain part's
    # no plain part, one relation given as Features; the twin's own expansion agrees
    one = RelationalData([1.0, 2.0], Relation(Features([0, 1, 3], [4, 2, 8], [1.0, 1.0, 0.5]), [1, 1]))
    assert one.expand().row_ptr.tolist() == [0, 2, 4] and one.expand().col.tolist() == [2, 8, 2, 8] and one.n_batches == 1
    p = rref.base_problem(3, 4)
    a = rref.flat(p)
    rels = [Relation((b["row_ptr"], b["col"], b["val"]), m) for b, m in zip(p["blocks"], p["maps"])]
    e = RelationalData(p["y"], rels, plain=Features(p["plain"]["row_ptr"], p["plain"]["col"], p["plain"]["val"])).expand()
    assert np.array_equal(e.row_ptr, a["row_ptr"]) and np.array_equal(e.col, a["col"]) and np.array_equal(e.val, a["val"])


# ---- symbols -----------------------------------------------------------------------------------------------------------

def test_header_matches_the_binding():
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_relational.h")).read()
    declared = set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_RELATIONAL) == {"fmhip_relational_" + n for n in ("create", "destroy", "info", "predict", "rmse", "logloss",
                                                                                        "sgd_step", "sgd_epoch")}
    others = (_ffi.SYMBOLS + _ffi.SYMBOLS_EXPERIMENTAL + _ffi.SYMBOLS_TOPK + _ffi.SYMBOLS_PAIRING + _ffi.SYMBOLS_METRICS + _ffi.SYMBOLS_RANKING
              + _ffi.SYMBOLS_WEIGHTS)
    assert not set(_ffi.SYMBOLS_RELATIONAL) & set(others)
    L = _ffi.load()
    for name in _ffi.SYMBOLS_RELATIONAL:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert int(re.search(r"#define FMHIP_RELATIONS_MAX (\d+)", hdr).group(1)) == _ffi.RELATIONS_MAX
    assert int(re.search(r"#define FMHIP_RELATIONAL_SUM_CUT (\d+)", hdr).group(1)) == _ffi.RELATIONAL_SUM_CUT
    assert {"fm_relational.hip", "fmhip_relational.hip"} <= set(_build.HIP_SOURCES) and "fm_relational.h" in _build.HIP_DEPS
    assert "relational" not in open(os.path.join(ROOT, "include", "fmhip.h")).read()          # fmhip.h stays as it is
    import sparkfm_amd
    assert sparkfm_amd.Relation and sparkfm_amd.RelationalData


# ---- refusals that need no device ------------------------------------------------------------------------------------------

def test_c_calls_refuse_null_arguments_without_a_device():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    y = np.zeros(3)
    h = C.c_void_p(7)
    blocks, maps = (C.c_void_p * 1)(None), (C.c_void_p * 1)(None)
    assert L.fmhip_relational_create(0, 3, _ffi.ptr(y), 1, blocks, maps, None, 0, None) == -1 and b"out is NULL" in L.fmhip_last_error()
    assert L.fmhip_relational_create(0, 3, None, 1, blocks, maps, None, 0, C.byref(h)) == -1 and h.value is None and b"y is NULL" in L.fmhip_last_error()
    assert L.fmhip_relational_create(0, 3, _ffi.ptr(y), 1, None, maps, None, 0, C.byref(h)) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_relational_create(0, 3, _ffi.ptr(y), 1, blocks, maps, None, 0, C.byref(h)) == -1 and b"relation 0: the block is NULL" in L.fmhip_last_error()
    assert L.fmhip_relational_create(0, 3, _ffi.ptr(y), 0, blocks, maps, None, 0, C.byref(h)) == -1 and b"n_relations = 0" in L.fmhip_last_error()
    assert L.fmhip_relational_create(0, 3, _ffi.ptr(y), 9, blocks, maps, None, 0, C.byref(h)) == -1 and b"1 .. 8" in L.fmhip_last_error()
    assert L.fmhip_relational_create(0, 0, _ffi.ptr(y), 1, blocks, maps, None, 0, C.byref(h)) == -1 and b"n_rows = 0" in L.fmhip_last_error()
    assert L.fmhip_relational_info(None, None, None, None, None, None) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_relational_destroy(None) == 0
    out, st = C.c_double(), _ffi.Stats()
    assert L.fmhip_relational_predict(None, None, None) == -1 and b"yhat is NULL" in L.fmhip_last_error()
    assert L.fmhip_relational_predict(None, None, _ffi.ptr(y)) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_relational_rmse(None, None, None, None) == -1 and b"rmse is NULL" in L.fmhip_last_error()
    assert L.fmhip_relational_rmse(None, None, C.byref(out), None) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_relational_logloss(None, None, C.byref(out), C.byref(st)) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_relational_sgd_step(None, None, 0, 0.1, 0.0, 0.0, 0.0, None) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_relational_sgd_epoch(None, None, 0.1, 0.0, 0.0, 0.0, None, None) == -1 and b"NULL" in L.fmhip_last_error()


def test_python_refuses_a_bad_mapping_and_a_shared_feature():
    from sparkfm_amd import DataSet, Relation, RelationalData
    users = [([1], [1.0]), ([2, 3], [0.5, 2.0])]
    items = [([5], [1.0]), ([6, 3], [1.0, 1.0])]                 # feature 3 is the users' too
    with pytest.raises(ValueError, match=r"relation 0: mapping\[2\] = 2 lies outside the block's rows \[0, 2\)"):
        RelationalData([1, 2, 3], [Relation(users, [0, 1, 2])])
    with pytest.raises(ValueError, match=r"relation 0: mapping\[1\] = -1"):
        RelationalData([1, 2, 3], [Relation(users, [0, -1, 5])])
    with pytest.raises(ValueError, match="feature 3 occurs in relation 0 and in relation 1"):
        RelationalData([1, 2], [Relation(users, [0, 1]), Relation(items, [1, 0])])
    plain = DataSet.from_rows([(0.0, ([6], [1.0])), (0.0, ([], []))])
    with pytest.raises(ValueError, match="feature 6 occurs in relation 1 and in the plain part"):
        RelationalData([1, 2], [Relation(users, [0, 1]), Relation([([5], [1.0]), ([6], [1.0])], [1, 0])], plain=plain)
    with pytest.raises(ValueError, match="the mapping holds 3 entries, the data has 2 rows"):
        RelationalData([1, 2], [Relation(users, [0, 1, 1])])
    with pytest.raises(ValueError, match="the plain part has 2 rows, the data 3"):
        RelationalData([1, 2, 3], [Relation(users, [0, 1, 1])], plain=plain)
    with pytest.raises(ValueError, match="at least one Relation"):
        RelationalData([1, 2], [])
    with pytest.raises(ValueError, match="integer"):
        Relation(users, [0.5, 1.0])


def test_other_calls_say_that_they_take_flat_rows():
    """Every call but HipSGD's and the four scores reaches for the dataset's flat handle: a RelationalData answers with a
    TypeError that says so — before any device call."""
    from sparkfm_amd import FMModel, HipALS, Relation, RelationalData
    rd = RelationalData([1.0, 2.0], [Relation([([1], [1.0]), ([2], [1.0])], [0, 1])])
    fm = FMModel(2, 2)
    fm._h, fm._dev_fresh = C.c_void_p(1), True                  # (no device: the handle is never used)
    try:
        for call in (lambda: fm.termQ(rd), lambda: fm.residual(rd), lambda: fm.computeAUC(rd), lambda: fm.batchGradient(rd),
                     lambda: fm.computePairLogLoss(rd), lambda: fm.weightedScores(rd), lambda: fm.recommend(rd, rd, 1),
                     lambda: fm.pairScores(rd, rd), lambda: HipALS().learn(fm, rd)):
            with pytest.raises(TypeError, match="RelationalData.*expand"):
                call()
    finally:
        fm._h = None


# ---- withRelation ----------------------------------------------------------------------------------------------------------

def test_with_relation_returns_self_and_accepts_a_list():
    from sparkfm_amd import FM, DataSet, Relation
    ds = DataSet(np.zeros(3, np.int64), [], [], [1.0, 2.0])
    u, i = Relation([([1], [1.0])], [0, 0]), Relation([([2], [1.0])], [0, 0])
    fm = FM(ds, 4)
    assert fm.withRelation(u) is fm and fm.relations == [u]
    assert fm.withRelation([i]) is fm and fm.relations == [u, i]
    assert FM(ds, 4).withRelation([u, i]).relations == [u, i]
    with pytest.raises(TypeError, match="Relation"):
        FM(ds, 4).withRelation("users")
    with pytest.raises(TypeError, match="Relation"):
        FM(ds, 4).withRelation([u, 3])


# ---- the host arithmetic under the sanitizers -------------------------------------------------------------------------------

def test_inverse_map_under_the_sanitizers(tmp_path):
    """tests/host_relational_harness.cpp with fmhip_host.cpp under AddressSanitizer and UBSan: a program of its own over seeded
    mappings (exactly n entries each) — empty lists, one list holding every row, J_b = 1, lists around the cut."""
    exe = str(tmp_path / "host_relational_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "host_relational_harness.cpp"), os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("no sanitizer runtime for g++ in this image")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    for seed in (20261019, 5):
        r = subprocess.run([exe, str(seed), "120"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
        assert r.returncode == 0 and b"checks ok" in r.stdout, (seed, r.stderr.decode()[-3000:])
