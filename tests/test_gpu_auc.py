"""ROC AUC and per-group AUC on the device (include/fmhip_metrics.h): fmhip_auc_scores through sparkfm_amd.metrics.auc with
crafted scores, fmhip_auc through FMModel.aucDetails over datasets of both kinds, against the numpy twin (auc_ref.py).

Every integer field must equal the twin's; auc must be u2 / (2.0 * pairs) exactly; gauc within 4 G 2^-53 relative of the twin's,
G = the number of groups (the fp64 reassociation of G non-negative terms: the twin sums them one by one, the device as a tree)."""
import ctypes as C
import math
import os
import subprocess
import threading

import numpy as np
import pytest

import oracle
from auc_ref import FIELDS, auc_ref, same
from helpers import random_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def agree(got, ref, what=""):
    """a result of the library against the twin's"""
    print(what, {k: got[k] for k in FIELDS + ("auc", "gauc")}, "twin gauc", ref["gauc"])
    for f in FIELDS:
        assert got[f] == ref[f], (what, f, got, ref)
    assert same(got["auc"], got["u2"] / (2.0 * got["pairs"]) if got["pairs"] else math.nan), (what, got)
    assert same(got["auc"], ref["auc"]), (what, got, ref)
    if math.isnan(ref["gauc"]):
        assert math.isnan(got["gauc"]), (what, got)
    else:
        assert abs(got["gauc"] - ref["gauc"]) <= 4 * ref["groups"] * 2.0 ** -53 * ref["gauc"], (what, got, ref)
    if got["groups_scored"] == 1:
        assert same(got["gauc"], got["auc"]), (what, got)


def check(fmhip, scores, labels, groups=None, what=""):
    from sparkfm_amd import metrics
    got = metrics.auc(scores, labels, groups)
    agree(got, auc_ref(scores, labels, groups), what)
    if groups is None:
        assert same(got["gauc"], got["auc"]) and got["groups"] == min(len(np.asarray(scores)), 1)
    return got


# ---- the core, with crafted scores

@pytest.mark.parametrize("n", [0, 1, 2, 255, 256, 257, 4097, 65537])
def test_sizes_with_block_and_tile_edges_inside_runs(fmhip, n):
    """Five distinct scores: the runs are long, so block and tile edges of every kernel and of the scans fall inside them."""
    rng = np.random.default_rng(n)
    s = rng.integers(0, 5, n).astype(np.float32) / 4
    y = (rng.random(n) < 0.3).astype(np.float32)
    check(fmhip, s, y, what="n=%d" % n)
    if n > 2:       # ... and with a few groups whose sizes are odd
        check(fmhip, s, y, rng.integers(0, 3, n) * 1000003, what="n=%d grouped" % n)


def test_all_scores_equal_is_one_run(fmhip):
    n = 70001
    y = (np.random.default_rng(1).random(n) < 0.5).astype(np.float32)
    r = check(fmhip, np.full(n, 0.75, np.float32), y)
    assert r["auc"] == 0.5 and r["u2"] == r["pairs"] == r["positives"] * r["negatives"]


def test_all_scores_distinct(fmhip):
    n = 30011
    rng = np.random.default_rng(2)
    s = (rng.permutation(n).astype(np.float32) - n // 2) / 64
    y = (rng.random(n) < 0.1).astype(np.float32)
    r = check(fmhip, s, y)
    assert r["u2"] % 2 == 0                     # no ties: every pair counts 0 or 2
    # a perfect ranking and its reverse
    assert check(fmhip, s, (s > 100).astype(np.float32))["auc"] == 1.0
    assert check(fmhip, -s, (s > 100).astype(np.float32))["auc"] == 0.0


def test_special_values_rank_by_the_stated_rule(fmhip):
    """-0 ties with +0, +-Inf rank as themselves, NaN below -Inf and equal to NaN."""
    vals = np.array([-np.inf, -1.5, -0.0, 0.0, 0.25, 3.0, np.inf, np.nan, -np.nan, 1e-45, -1e-45], np.float32)
    rng = np.random.default_rng(3)
    s = vals[rng.integers(0, len(vals), 3001)]
    y = (rng.random(3001) < 0.5).astype(np.float32)
    check(fmhip, s, y)
    check(fmhip, s, y, rng.integers(0, 40, 3001))
    from sparkfm_amd import metrics
    assert metrics.auc([-0.0, 0.0], [1, 0])["u2"] == 1                        # a tie
    assert metrics.auc([np.nan, -np.inf], [1, 0])["u2"] == 0                  # NaN below -Inf
    assert metrics.auc([np.nan, np.nan], [1, 0])["u2"] == 1                   # NaN ties with NaN
    assert metrics.auc([np.inf, 3e38, -np.inf], [1, 0, 0])["u2"] == 4


def test_one_class_only(fmhip):
    s = np.random.default_rng(4).normal(size=1000).astype(np.float32)
    for y in (np.ones(1000, np.float32), np.zeros(1000, np.float32), -np.ones(1000, np.float32)):
        r = check(fmhip, s, y)
        assert r["pairs"] == 0 and r["u2"] == 0 and r["groups"] == 1 and r["groups_scored"] == 0
        assert math.isnan(r["auc"]) and math.isnan(r["gauc"])


def test_labels_plus_minus_one_and_zero_one(fmhip):
    rng = np.random.default_rng(5)
    s = rng.integers(-3, 4, 5003).astype(np.float32)
    t = rng.random(5003) < 0.4
    a = check(fmhip, s, np.where(t, 1.0, -1.0))
    b = check(fmhip, s, np.where(t, 1.0, 0.0))
    c = check(fmhip, s, np.where(t, 0.5, -0.0))
    assert a == b == c or all(same(a[k], b[k]) and same(a[k], c[k]) for k in a)


# ---- groups

def test_every_row_its_own_group(fmhip):
    n = 1000
    rng = np.random.default_rng(6)
    r = check(fmhip, rng.normal(size=n).astype(np.float32), (rng.random(n) < 0.5).astype(np.float32), rng.permutation(n) * 7)
    assert r["groups"] == n and r["groups_scored"] == 0 and math.isnan(r["auc"]) and math.isnan(r["gauc"])


def test_two_groups_one_with_a_single_class(fmhip):
    s = np.array([0.1, 0.9, 0.5, 0.5, 0.2, 0.7, 0.3], np.float32)
    y = np.array([0, 1, 1, 0, 1, 1, 1], np.float32)
    g = np.array([5, 5, 5, 5, 2, 2, 2])
    r = check(fmhip, s, y, g)
    assert (r["groups"], r["groups_scored"], r["pairs"], r["u2"]) == (2, 1, 4, 2 + 2 + 2 + 1)
    assert r["gauc"] == r["auc"] == 7 / 8


def test_ten_thousand_uneven_groups(fmhip):
    n = 60001
    rng = np.random.default_rng(7)
    g = np.minimum(rng.zipf(1.3, n), 10 ** 4) * 211 + 5          # sparse ids, a few very large groups and thousands of tiny ones
    s = rng.integers(0, 50, n).astype(np.float32)
    y = (rng.random(n) < 0.3).astype(np.float32)
    r = check(fmhip, s, y, g)
    assert 3000 < r["groups"] <= 10 ** 4 and 0 < r["groups_scored"] < r["groups"]


def test_sparse_unsorted_ids_with_the_extremes(fmhip):
    rng = np.random.default_rng(8)
    ids = np.array([2 ** 31 - 1, 0, 2 ** 30, 1, 123456789, 2 ** 31 - 2])
    g = ids[rng.integers(0, len(ids), 4099)]
    r = check(fmhip, rng.integers(0, 9, 4099).astype(np.float32), (rng.random(4099) < 0.5).astype(np.float32), g)
    assert r["groups"] == r["groups_scored"] == 6


def test_negative_group_id_is_refused(fmhip):
    from sparkfm_amd import _ffi, metrics
    g = np.zeros(5000, np.int64)
    g[4321] = -1
    with pytest.raises(_ffi.FmhipError, match="row 4321") as e:
        metrics.auc(np.zeros(5000, np.float32), np.ones(5000, np.float32), g)
    assert e.value.code == -1


def test_group_heads_on_tile_edges(fmhip):
    """Group sizes that are multiples of 256 (and of the scans' larger tiles), in ascending id order, so that group heads and
    run heads fall on the first position of a block; then the same shifted by one row."""
    sizes = [256, 256, 512, 1024, 2048, 4096, 256, 1, 255, 8192, 3840, 256]
    g = np.repeat(np.arange(len(sizes)) * 3, sizes)
    rng = np.random.default_rng(9)
    s = rng.integers(0, 3, len(g)).astype(np.float32)
    y = (rng.random(len(g)) < 0.5).astype(np.float32)
    check(fmhip, s, y, g)
    check(fmhip, s[1:], y[1:], g[1:])
    check(fmhip, np.zeros(len(g), np.float32), y, g)              # one run per group: run heads == group heads


# ---- a model over a dataset

def logistic_problem(seed, n_rows, n1, k, stdev=0.1):
    a = random_problem(seed, n_rows, n1, k, 0, 30, empty_rows=(0, 17, n_rows - 1), scale=stdev)
    a["y"] = np.where(np.random.default_rng(seed + 1).random(n_rows) < 0.4, 1.0, 0.0)
    return a


def model_of(fmhip, a, loss="logistic"):
    from sparkfm_amd import _ffi
    fm = fmhip.FMModel(a["n1"] - 1, a["k"])
    fm.w0, fm.w, fm.v = a["w0"], a["w"], a["v"]
    _ffi.check(_ffi.load().fmhip_model_set_loss(fm.handle, _ffi.loss_code(loss)))
    return fm


def ranks_what_predict_returns(fm, ds, groups, what):
    """aucDetails == the twin applied to fm.predict(ds) and the labels: it ranks exactly the bits predict returns"""
    yh = fm.predict(ds)
    assert (yh == yh.astype(np.float32)).all()
    got = fm.aucDetails(ds, groups, stats=True)
    st = got.pop("stats")
    agree(got, auc_ref(yh, ds.y, groups), what)
    assert same(fm.computeAUC(ds, groups), got["auc"])
    if groups is not None:
        assert same(fm.computeGroupAUC(ds, groups), got["gauc"])
    return got, st


@pytest.mark.parametrize("k", [8, 32])
def test_model_over_training_and_scoring_datasets(fmhip, k):
    """A small logistic model, 2500 rows: a scoring-only dataset, and a training dataset of three batches with the last one
    partial; ungrouped and with ~300 groups; stats are fmhip_rmse's."""
    from sparkfm_amd import _ffi
    a = logistic_problem(40 + k, 2500, 300, k)
    fm = model_of(fmhip, a)
    g = np.random.default_rng(k).integers(0, 300, 2500) * 7919
    results = []
    for kw in (dict(scoring=True), dict(batch_rows=1000)):
        ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], **kw).cache()
        assert ds.n_batches == (3 if "batch_rows" in kw else ds.n_batches)
        for groups in (None, g):
            got, st = ranks_what_predict_returns(fm, ds, groups, "k=%d %s" % (k, kw))
            results.append(got)
            ref = _ffi.Stats()
            rmse = C.c_double()
            _ffi.check(_ffi.load().fmhip_rmse(fm.handle, ds.handle, C.byref(rmse), C.byref(ref)))
            assert st == ref.as_dict() and st["rows"] == 2500 and st["nonfinite"] == 0
        ds.unpersist()
    # the two kinds of dataset hold the same rows: the same answer
    assert all(same(results[0][f], results[2][f]) and same(results[1][f], results[3][f]) for f in results[0])
    assert 0.0 < results[0]["auc"] < 1.0 and results[1]["groups"] <= 300
    fm.close()


def test_scoring_dataset_across_the_internal_batch(fmhip):
    """262 144 + 3 rows of two entries each: more than one internal scoring batch, the last one of three rows."""
    n, n1 = 262144 + 3, 64
    rng = np.random.default_rng(11)
    a = dict(n1=n1, k=8, w0=0.05, w=rng.normal(0, 0.1, n1), v=rng.normal(0, 0.1, (8, n1)))
    col = np.stack([rng.integers(0, 32, n), rng.integers(32, 64, n)], axis=1).reshape(-1).astype(np.int32)
    ds = fmhip.DataSet(np.arange(n + 1, dtype=np.int64) * 2, col, np.ones(2 * n), (rng.random(n) < 0.2).astype(np.float64),
                       scoring=True).cache()
    assert ds.n_batches > 1
    fm = model_of(fmhip, a)
    got, st = ranks_what_predict_returns(fm, ds, None, "262147 rows")       # (32 x 32 distinct rows: long runs)
    assert st["rows"] == n
    ranks_what_predict_returns(fm, ds, rng.integers(0, 5000, n), "262147 rows grouped")
    ds.unpersist()
    fm.close()


def test_lazily_decayed_model(fmhip):
    """A wide model whose step takes the rows-only update with lazy decay (the tables then hold U with V = sv U): the AUC call
    ranks what predict returns before the step and after it, and the step moved the predictions."""
    a = logistic_problem(51, 800, 20000, 64)
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=100).cache()
    fm = model_of(fmhip, a)
    g = np.arange(800) % 37
    before, _ = ranks_what_predict_returns(fm, ds, g, "before the step")
    y0 = fm.predict(ds)
    sgd = fmhip.HipSGD(eta=0.1, reg0=1e-3, regw=1e-3, regv=2e-3, loss="logistic")
    sgd.step(fm, ds, 0)
    assert (fm.predict(ds) != y0).any()
    after, _ = ranks_what_predict_returns(fm, ds, g, "after the step")
    assert after["positives"] == before["positives"] and after["groups"] == before["groups"] == 37
    again = fm.aucDetails(ds, g)
    assert all(same(again[f], after[f]) for f in again)                       # repeated calls: identical bits
    ds.unpersist()
    fm.close()


def test_against_the_fp64_oracle(fmhip):
    """Only the pairs whose fp64 margin |yhat_p - yhat_n| is within the two rows' parity tolerances, tol_r = 1e-5 (1 + sum |terms|)
    (test_gpu_parity.py) — twice the tolerance for rows of equal scale — can be ordered differently in fp32, and each by at most
    one pair's worth: |AUC - AUC_oracle| <= their share of the pairs.  The model is drawn with stdev 0.1 so that the share is
    small: below 1 % (a condition on the input, checked on the oracle alone)."""
    from test_gpu_parity import TOL_Y, term_scale
    a = logistic_problem(61, 2500, 300, 16, stdev=0.1)
    oyh = oracle.predict(a["w0"], a["w"], a["v"], a["row_ptr"], a["col"], a["val"])
    tol = TOL_Y * term_scale(a)
    t = a["y"] > 0
    d = oyh[t][:, None] - oyh[~t][None, :]
    auc_oracle = ((d > 0).sum() + 0.5 * (d == 0).sum()) / d.size
    share = (np.abs(d) <= tol[t][:, None] + tol[~t][None, :]).sum() / d.size
    print("oracle AUC", auc_oracle, "share of the pairs that may flip", share)
    assert share < 0.01
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], scoring=True).cache()
    fm = model_of(fmhip, a)
    got = fm.computeAUC(ds)
    print("device AUC", got, "difference", abs(got - auc_oracle))
    assert abs(got - auc_oracle) <= share
    ds.unpersist()
    fm.close()


# ---- other checks

def test_zero_model_with_negative_zero_bias_ties_every_row(fmhip):
    """w0 = -0.0, w = 0, v = 0, one empty positive row and non-empty negative rows with entries of either sign: every prediction
    is a zero of one sign or the other, and all of them tie."""
    n1, k, n = 50, 8, 300
    rng = np.random.default_rng(12)
    a = random_problem(12, n, n1, k, 1, 6, empty_rows=(0,))
    a.update(w0=-0.0, w=np.zeros(n1), v=np.zeros((k, n1)), y=np.concatenate([[1.0], np.zeros(n - 1)]))
    a["val"] = a["val"] * rng.choice([-1.0, 1.0], len(a["val"]))
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], scoring=True).cache()
    fm = model_of(fmhip, a, "squared")
    yh = fm.predict(ds)
    assert (yh == 0).all()
    print("signs of the zeros:", sorted(set(np.copysign(1.0, yh).tolist())))
    r = fm.aucDetails(ds)
    assert r["auc"] == 0.5 and r["u2"] == r["pairs"] == n - 1 and r["gauc"] == 0.5
    ds.unpersist()
    fm.close()


def test_two_threads_score_one_model_at_once(fmhip):
    a = logistic_problem(71, 2500, 300, 32)
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=1000).cache()
    fm = model_of(fmhip, a)
    g = np.random.default_rng(13).integers(0, 100, 2500)
    fm.handle, ds.handle                                                       # (uploaded before the threads start)
    alone = fm.aucDetails(ds, g)
    out = [[], []]

    def work(i):
        for _ in range(5):
            out[i].append(fm.aucDetails(ds, g))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for r in out[0] + out[1]:
        assert len(out[0]) == len(out[1]) == 5 and all(same(r[f], alone[f]) for f in alone), (r, alone)
    ds.unpersist()
    fm.close()


def test_cpp_mirror_prints_the_same_integers(fmhip, tmp_path):
    """include/sparkfm.hpp's computeAUC / computeGroupAUC / aucDetails (tests/cpp_auc.cpp) on a problem both sides build from the
    same integer recipe: the Python mirror's integers, and the two ratios bit for bit."""
    from sparkfm_amd import _build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_auc")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_auc.cpp"), "-L" + _build.LIBDIR, "-lfmhip",
                           "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    lines = [ln.split() for ln in r.stdout.decode().split("\n") if ln.strip()]
    assert len(lines) == 2
    # the recipe of tests/cpp_auc.cpp
    N, n1, k = 600, 96, 6
    w = np.array([((i * 7) % 11 - 5) / 32.0 for i in range(n1)])
    v = np.array([[((f * 5 + i * 3) % 13 - 6) / 40.0 for i in range(n1)] for f in range(k)])
    ptr, col, val, y, g = [0], [], [], [], []
    for row in range(N):
        if row % 10 != 3:
            for j in range(1 + row % 3):
                col.append((row * 5 + j * 17) % 32 + 32 * j)
                val.append(1.0 if (row + j) % 2 else 0.5)
        ptr.append(len(col))
        y.append(1.0 if (row * 7) % 5 < 2 else -1.0)
        g.append(2147483647 if (row * 13) % 41 == 0 else (row * 13) % 41)
    ds = fmhip.DataSet(np.array(ptr, np.int64), np.array(col, np.int32), np.array(val), np.array(y), batch_rows=250).cache()
    fm = fmhip.FMModel(n1 - 1, k)
    fm.w0, fm.w, fm.v = -0.0625, w, v
    for ln, groups in zip(lines, (None, np.array(g))):
        py = fm.aucDetails(ds, groups)
        assert [int(x) for x in ln[:6]] == [py[f] for f in FIELDS]
        assert same(float.fromhex(ln[6]), py["auc"]) and same(float.fromhex(ln[7]), py["gauc"])
        agree(py, auc_ref(fm.predict(ds), y, groups), "cpp recipe")
    assert int(lines[1][4]) == 41 and int(lines[0][4]) == 1
    ds.unpersist()
    fm.close()


def test_trained_model_beats_chance_on_planted_data(fmhip):
    """A sanity check, not parity: labels planted by a hidden linear rule, twenty epochs of logistic SGD; AUC and GAUC on held-out
    rows beat the 0.5 of a model that cannot tell the classes apart (by 0.1: 1000 rows put chance within +-0.03)."""
    n, n1, k = 4000, 200, 8
    a = random_problem(81, n, n1, k, 4, 12, scale=0.01)
    hidden = np.random.default_rng(82).normal(0, 1.0, n1)
    margin = np.array([(hidden[a["col"][a["row_ptr"][r]:a["row_ptr"][r + 1]]] * a["val"][a["row_ptr"][r]:a["row_ptr"][r + 1]]).sum()
                       for r in range(n)])
    a["y"] = (margin > 0).astype(np.float64)
    a.update(w0=0.0, w=np.zeros(n1))
    train = fmhip.DataSet(a["row_ptr"][:3001], a["col"][:a["row_ptr"][3000]], a["val"][:a["row_ptr"][3000]], a["y"][:3000],
                          batch_rows=500).cache()
    rp = a["row_ptr"][3000:] - a["row_ptr"][3000]
    test = fmhip.DataSet(rp, a["col"][a["row_ptr"][3000]:], a["val"][a["row_ptr"][3000]:], a["y"][3000:], scoring=True).cache()
    fm = model_of(fmhip, a)
    g = np.arange(1000) % 20
    start = fm.aucDetails(test, g)
    sgd = fmhip.HipSGD(eta=0.5, loss="logistic")
    for _ in range(20):
        sgd.learn(fm, train)
    end = fm.aucDetails(test, g)
    print("AUC", start["auc"], "->", end["auc"], "GAUC", start["gauc"], "->", end["gauc"])
    assert end["auc"] > 0.6 and end["gauc"] > 0.6 and end["groups_scored"] == 20
    train.unpersist()
    test.unpersist()
    fm.close()
