"""Parity of the HIP path (through the C ABI) against the CPU oracle and the KATs.

Tolerances (fp32 device arithmetic vs the fp64 oracle on identical inputs):
  index gathers / transposes : bit-exact
  yhat, e                    : |d| <= 1e-5 * (1 + sum|terms|)     (TOL_Y)
  RMSE                       : rel 1e-5
  one-step gradient          : per feature row, |d| <= 1e-4 * max(|G[i,:]|inf, scale)  (TOL_G)
  parameters after T <= 20 steps: rel-L2 <= 1e-4 (measured ~1e-6; SURVEY proposed 1e-3)
"""
import math
import os

import numpy as np
import pytest

import oracle
from sparkfm_amd import _ffi  # noqa: F401  (the tuning keys' names)
from helpers import f, kat_arrays, random_problem

pytestmark = pytest.mark.gpu

TOL_Y = 1e-5
TOL_G = 1e-4


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def torch_stream():
    """The dedicated torch stream HipEngine requires the model to run on (made current on first use)."""
    from sparkfm_amd.distributed import torch_stream_handle
    return torch_stream_handle(0)


def make(fmhip, a, batch_rows=0, stream=None):
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=batch_rows).cache()
    fm = fmhip.FMModel(a["n1"] - 1, a["k"], stream=stream)
    fm.w0, fm.w, fm.v = a["w0"], a["w"], a["v"]
    return ds, fm


def term_scale(a):
    """1 + sum of |terms| of the forward per row (for the yhat tolerance)."""
    n_rows = len(a["y"])
    out = np.ones(n_rows)
    for r in range(n_rows):
        s = slice(a["row_ptr"][r], a["row_ptr"][r + 1])
        idx, x = a["col"][s], a["val"][s]
        t = np.abs(a["v"][:, idx] * x)
        out[r] += abs(a["w0"]) + np.abs(a["w"][idx] * x).sum() + 0.5 * ((t.sum(axis=1) ** 2).sum() + (t * t).sum())
    return out


def check_grad(gv, gw, ogv, ogw, vmax=1.0, cancelled=0.0, terms=None, w_terms=None):
    # the V gradient is a difference of two sums (sum e*x*q  -  v * sum e*x^2) that can cancel
    # exactly (single-nonzero rows): the floor is set by the size of the cancelled terms — `cancelled` = max over the
    # features of sum |e*x| (when the caller has the residuals), else the signed sums in ogw stand in for it
    scale = max(np.abs(ogv).max(), np.abs(ogw).max() * vmax, cancelled * vmax, 1e-6)
    rowmax = np.maximum(np.abs(ogv).max(axis=0), 1e-3 * scale)
    tol = TOL_G * rowmax
    if terms is not None:
        # fp32 summation of a feature's terms: a few ulps of the sum of their magnitudes, whatever cancels in the total
        tol = tol + 2e-6 * np.asarray(terms)
    assert (np.abs(gv - ogv) <= tol[None, :]).all(), float((np.abs(gv - ogv) / tol[None, :]).max())
    if w_terms is None:
        np.testing.assert_allclose(gw, ogw, rtol=TOL_G, atol=TOL_G * max(np.abs(ogw).max(), 1e-6))
    else:
        tolw = TOL_G * np.maximum(np.abs(ogw), max(np.abs(ogw).max(), 1e-6)) + 2e-6 * np.asarray(w_terms)
        assert (np.abs(gw - ogw) <= tolw).all(), float((np.abs(gw - ogw) / tolw).max())


def test_kats_through_the_c_abi(fmhip, kats):
    for c in kats:
        a = kat_arrays(c)
        ds, fm = make(fmhip, a)
        sc = term_scale(a)
        yh = fm.predict(ds)
        assert (np.abs(yh - np.array(f(c["yhat"]))) <= TOL_Y * sc).all()
        e = fm.residual(ds)
        assert (np.abs(e - np.array(f(c["e"]))) <= TOL_Y * sc).all()
        assert fm.computeRMSE(ds) == pytest.approx(math.sqrt(f(c["mse"])), rel=1e-5)
        np.testing.assert_allclose(fm.termQ(ds), np.array(f(c["q"])), rtol=1e-5, atol=1e-6)
        gv, gw, g0, st = fm.batchGradient(ds, 0)
        check_grad(gv, gw, np.array(f(c["grad"]["gV"])), np.array(f(c["grad"]["gw"])), np.abs(a["v"]).max())
        assert g0 == pytest.approx(f(c["grad"]["g0"]), rel=1e-5, abs=1e-6)
        assert st["sse"] == pytest.approx(f(c["sse"]), rel=1e-5)
        s = c["sgd"]
        sgd = fmhip.HipSGD(eta=f(s["eta"]), reg0=f(s["reg0"]), regw=f(s["regw"]), regv=f(s["regv"]))
        sgd.step(fm, ds, 0)
        np.testing.assert_allclose(fm.v, np.array(f(s["V"])), rtol=2e-6, atol=2e-7)
        np.testing.assert_allclose(fm.w, f(s["w"]), rtol=2e-6, atol=2e-7)
        assert fm.w0 == pytest.approx(f(s["w0"]), rel=2e-6, abs=2e-7)
        ds.unpersist()
        fm.close()


@pytest.mark.parametrize("k", [1, 2, 3, 4, 8, 16, 32, 33, 64, 100, 128])
def test_forward_and_gradient_vs_oracle(fmhip, k):
    # 4 ragged batches; empty rows; unsorted indices; a feature (id 0) present in every non-empty row
    a = random_problem(100 + k, 1000, 257, k, 0, 40, empty_rows=(0, 17, 999))
    for r in range(1000):
        s = slice(a["row_ptr"][r], a["row_ptr"][r + 1])
        if s.stop > s.start and not (a["col"][s] == 0).any():
            a["col"][s.start] = 0
    ds, fm = make(fmhip, a, batch_rows=300)
    assert ds.info() == dict(n_rows=1000, nnz=int(a["row_ptr"][-1]), dimension=int(a["col"].max()), batch_rows=300,
                             n_batches=4)
    sc = term_scale(a)
    yh = fm.predict(ds)
    oyh = oracle.predict(a["w0"], a["w"], a["v"], a["row_ptr"], a["col"], a["val"])
    assert (np.abs(yh - oyh) <= TOL_Y * sc).all(), float((np.abs(yh - oyh) / sc).max())
    for r in (0, 17, 999):
        assert yh[r] == np.float32(a["w0"])                       # empty row -> w0 exactly (quirk Q6)
    assert fm.computeRMSE(ds) == pytest.approx(oracle.rmse(a["w0"], a["w"], a["v"], a["row_ptr"], a["col"], a["val"],
                                                           a["y"]), rel=1e-5)
    q = fm.termQ(ds)
    cp, rows, cv = oracle.transpose(a["n1"], a["row_ptr"], a["col"], a["val"])
    for ff in range(0, k, max(1, k // 3)):
        np.testing.assert_allclose(q[:, ff], oracle.term_q(a["v"], ff, 1000, cp, rows, cv), rtol=1e-5, atol=1e-5)
    for b in range(4):
        r0, r1 = b * 300, min(1000, (b + 1) * 300)
        gv, gw, g0, st = fm.batchGradient(ds, b)
        ogv, ogw, og0, osse, oe = oracle.batch_grad(a["w0"], a["w"], a["v"], r0, r1, a["row_ptr"], a["col"], a["val"],
                                                    a["y"])
        check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
        assert g0 == pytest.approx(og0, rel=1e-5, abs=1e-4)
        assert st["sse"] == pytest.approx(osse, rel=1e-5)
        assert st["rows"] == r1 - r0 and st["nonfinite"] == 0
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("window", ["0", "64", "100"])
def test_forward_walk_order_is_only_an_order(fmhip, monkeypatch, window):
    """Wide rows (Kp >= 64) are walked longest-first; FMHIP_ORDER_WINDOW (an experiment knob read when the dataset is built)
    sorts inside windows of rows instead.  Whatever the order, every row is visited once: predictions, residual
    statistics and the gradient are the oracle's."""
    monkeypatch.setenv("FMHIP_ORDER_WINDOW", window)
    a = random_problem(777, 1500, 300, 64, 0, 60, empty_rows=(3, 1499))
    ds, fm = make(fmhip, a, batch_rows=700)
    sc = term_scale(a)
    yh = fm.predict(ds)
    oyh = oracle.predict(a["w0"], a["w"], a["v"], a["row_ptr"], a["col"], a["val"])
    assert (np.abs(yh - oyh) <= TOL_Y * sc).all()
    assert yh[3] == np.float32(a["w0"]) and yh[1499] == np.float32(a["w0"])
    gv, gw, g0, st = fm.batchGradient(ds, 1)
    ogv, ogw, og0, osse, oe = oracle.batch_grad(a["w0"], a["w"], a["v"], 700, 1400, a["row_ptr"], a["col"], a["val"], a["y"])
    check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
    assert st["sse"] == pytest.approx(osse, rel=1e-5) and st["rows"] == 700
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("fwd,bwd,tile", [(20, 1, 0), (20, 1, 16), (0, 0, 0), (60, 1, 0), (60, 1, 50)])
def test_kernel_variants_agree_with_the_oracle(fmhip, fwd, bwd, tile):
    """fmhip_tune: the LDS V-tile forward (ids < tile rows come from LDS, the rest from global
    memory) and the plain backward walk give the same results as the default kernels."""
    from sparkfm_amd import _ffi
    L = _ffi.load()
    try:
        L.fmhip_tune(_ffi.TUNE_FORWARD_KERNEL, fwd), L.fmhip_tune(_ffi.TUNE_BACKWARD_KERNEL, bwd), L.fmhip_tune(_ffi.TUNE_TILE_ROWS, tile)
        for k in (8, 32, 64, 128):
            a = random_problem(300 + k, 700, 300, k, 0, 30, empty_rows=(1, 699))
            ds, fm = make(fmhip, a, batch_rows=256)
            sc = term_scale(a)
            yh = fm.predict(ds)
            oyh = oracle.predict(a["w0"], a["w"], a["v"], a["row_ptr"], a["col"], a["val"])
            assert (np.abs(yh - oyh) <= TOL_Y * sc).all()
            gv, gw, g0, st = fm.batchGradient(ds, 1)
            ogv, ogw, og0, osse, _ = oracle.batch_grad(a["w0"], a["w"], a["v"], 256, 512, a["row_ptr"], a["col"],
                                                       a["val"], a["y"])
            check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
            assert st["sse"] == pytest.approx(osse, rel=1e-5)
            sgd = fmhip.HipSGD(eta=0.03, regv=1e-3)
            sgd.learn(fm, ds)
            w0, w, v, sse = oracle.sgd_epoch(a["w0"], a["w"], a["v"], 256, a["row_ptr"], a["col"], a["val"], a["y"],
                                             0.03, 0.0, 0.0, 1e-3)
            assert np.linalg.norm(fm.v - v) <= 1e-5 * np.linalg.norm(v)
            assert sgd.last_stats["sse"] == pytest.approx(sse, rel=1e-5)
            ds.unpersist()
            fm.close()
    finally:
        L.fmhip_tune(_ffi.TUNE_FORWARD_KERNEL, 60), L.fmhip_tune(_ffi.TUNE_BACKWARD_KERNEL, 1), L.fmhip_tune(_ffi.TUNE_TILE_ROWS, 0)


@pytest.mark.parametrize("rb", [64, 100, 1000])
def test_row_blocked_transposes(fmhip, rb):
    """fmhip_tune(_ffi.TUNE_ROW_BLOCK, rb): the batch transposes are sorted by (row block of `rb` rows, feature); a
    feature occurring in several blocks is cut into pieces summed by k_fixup2.  Same gradient (to fp32
    reassociation), same transposes through the read-back API, deterministic."""
    from sparkfm_amd import _ffi
    L = _ffi.load()
    try:
        L.fmhip_tune(_ffi.TUNE_ROW_BLOCK, rb)
        for k in (8, 32, 64, 200):
            a = random_problem(700 + k, 900, 150, k, 0, 25, empty_rows=(2, 450))
            for r in range(900):                                    # feature 1 in (almost) every row: many pieces
                s = slice(a["row_ptr"][r], a["row_ptr"][r + 1])
                if s.stop > s.start and not (a["col"][s] == 1).any():
                    a["col"][s.start] = 1
            a["val"] = a["val"].astype(np.float32).astype(np.float64)
            ds, fm = make(fmhip, a, batch_rows=400)
            for b in range(3):
                r0, r1 = b * 400, min(900, (b + 1) * 400)
                sub = a["row_ptr"][r0:r1 + 1] - a["row_ptr"][r0]
                sl = slice(a["row_ptr"][r0], a["row_ptr"][r1])
                cp, rows, cv = oracle.transpose(a["n1"], sub, a["col"][sl], a["val"][sl])
                feat, ptr, drows, dvals = ds.transposeInput(b)
                present = np.nonzero(np.diff(cp))[0]
                np.testing.assert_array_equal(feat, present.astype(np.int32))
                np.testing.assert_array_equal(drows, rows)
                np.testing.assert_array_equal(dvals.astype(np.float64), cv)
                gv, gw, g0, st = fm.batchGradient(ds, b)
                ogv, ogw, og0, osse, _ = oracle.batch_grad(a["w0"], a["w"], a["v"], r0, r1, a["row_ptr"], a["col"],
                                                           a["val"], a["y"])
                check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
                gv2, gw2, _, _ = fm.batchGradient(ds, b)
                np.testing.assert_array_equal(gv, gv2)
            sgd = fmhip.HipSGD(eta=0.03, regv=1e-3)
            sgd.learn(fm, ds)
            w0, w, v, sse = oracle.sgd_epoch(a["w0"], a["w"], a["v"], 400, a["row_ptr"], a["col"], a["val"], a["y"],
                                             0.03, 0.0, 0.0, 1e-3)
            assert np.linalg.norm(fm.v - v) <= 1e-5 * np.linalg.norm(v)
            ds.unpersist()
            fm.close()
    finally:
        L.fmhip_tune(_ffi.TUNE_ROW_BLOCK, 0)


def hot_problem(seed, n_rows, n1, k, n_hot, dup_feature=None, zero_feature=None, n_low=0):
    """Rows over n1 features of which the first n_hot (scattered over the id range) occur in 15-95 % of
    the rows (the last n_low of them in 6.5-9 % only: dense on the gradient side, never in page 0); optionally one hot
    feature occurs twice in some rows / is stored with explicit zeros."""
    rng = np.random.default_rng(seed)
    hot_ids = np.sort(rng.choice(n1, size=n_hot, replace=False))
    freq = rng.uniform(0.15, 0.95, n_hot)
    if n_low:
        freq[n_hot - n_low:] = rng.uniform(0.065, 0.09, n_low)
    cold = np.setdiff1d(np.arange(n1), hot_ids)
    rows, vals = [], []
    for r in range(n_rows):
        idx = list(hot_ids[rng.random(n_hot) < freq])
        idx += list(rng.choice(cold, size=int(rng.integers(0, 6)), replace=False))
        x = list(rng.uniform(0.1, 1.0, len(idx)))
        if dup_feature is not None and r % 7 == 0:
            idx.append(hot_ids[dup_feature]); x.append(0.5)
        if zero_feature is not None and r % 5 == 0 and hot_ids[zero_feature] not in idx:
            idx.append(hot_ids[zero_feature]); x.append(0.0)
        perm = rng.permutation(len(idx))
        rows.append(np.asarray(idx, np.int32)[perm]); vals.append(np.asarray(x)[perm])
    for f_ in hot_ids[n_hot - n_low:]:
        # a feature drawn at <= 9 % can still reach 10 % of the rows by chance (seed 556: 406 of 4000), and then it belongs in
        # page 0: take it out of the rows past the (n_rows - 1) // 10-th that hold it, so that it stays below the mark
        has = [r for r in range(n_rows) if (rows[r] == f_).any()]
        for r in has[(n_rows - 1) // 10:]:
            keep = rows[r] != f_
            rows[r], vals[r] = rows[r][keep], vals[r][keep]
    row_ptr = np.zeros(n_rows + 1, np.int64)
    row_ptr[1:] = np.cumsum([len(r) for r in rows])
    return dict(k=k, n1=n1, w0=0.25, w=rng.normal(0, 0.1, n1), v=rng.normal(0, 0.1, (k, n1)), row_ptr=row_ptr,
                col=np.concatenate(rows), val=np.concatenate(vals), y=rng.normal(0, 1, n_rows)), hot_ids


@pytest.mark.parametrize("k,n_hot,dup,zero,pages", [(32, 16, None, None, 3), (32, 20, None, None, 3), (32, 20, None, None, 1),
                                                      (16, 5, None, None, 3), (64, 9, 2, None, 3), (100, 16, None, 3, 3),
                                                      (8, 12, 0, 1, 3), (32, 48, None, None, 3), (32, 41, 20, 30, 2),
                                                      (64, 45, 3, None, 3), (16, 35, None, 1, 3), (100, 40, 25, None, 3), (32, 70, 50, None, 4),
                                                      (64, 64, None, None, 4), (32, 100, None, None, 8), (64, 128, 5, None, 8),
                                                      (32, 90, 60, 70, 6), (200, 20, None, None, 3), (256, 40, 25, 30, 4),
                                                      (129, 16, 0, 1, 2)])
@pytest.mark.parametrize("flat", [0, 1])
def test_dense_hot_block(fmhip, request, k, n_hot, dup, zero, pages, flat):
    """fmhip_tune(_ffi.TUNE_HOT_BLOCK, 1): the most frequent features (>= 10 % of the rows, none that occurs twice in a row or with a stored
    zero) are held in dense [rows][16] pages: the 16 most frequent leave the sparse streams on both sides, up to 112 more
    (fmhip_tune key 12 = pages, at most 8) leave the transposes only and get their gradient rows from the same MFMA block
    product.  Forward, gradient, transposes, epochs and the feature-chunked backward must not notice.  k <= 32 forms all 8
    pages in one pass over P, k = 64 four pages per pass (so 8 pages take two), k = 100 (Kp = 128) one pass per page.  flat=1: the same on the flat-address kernels (fmhip_tune key 8)."""
    from sparkfm_amd import _ffi
    L = _ffi.load()
    L.fmhip_tune(_ffi.TUNE_FLAT_ADDRESS, flat)
    request.addfinalizer(lambda: L.fmhip_tune(_ffi.TUNE_FLAT_ADDRESS, 0))
    a, hot_ids = hot_problem(100 + k, 3000, 500, k, n_hot, dup, zero)
    a["val"] = a["val"].astype(np.float32).astype(np.float64)       # exactly representable in fp32
    n_rows, br = 3000, 700
    try:
        L.fmhip_tune(_ffi.TUNE_HOT_BLOCK, 1)
        L.fmhip_tune(_ffi.TUNE_HOT_PAGES, pages)
        ds, fm = make(fmhip, a, batch_rows=br)
    finally:
        L.fmhip_tune(_ffi.TUNE_HOT_BLOCK, 1)
        L.fmhip_tune(_ffi.TUNE_HOT_PAGES, 4)
    lay = ds.layout()
    refused = {int(hot_ids[i]) for i in (dup, zero) if i is not None}
    dense = set(lay["hot_ids_all"])
    assert dense <= {int(x) for x in hot_ids} - refused and set(lay["hot_ids"]) <= dense
    assert len(dense) == min(n_hot - len(refused), 16 * pages) and lay["hot_pages"] == (len(dense) + 15) // 16
    assert lay["nnz_sparse_backward"] == int((~np.isin(a["col"], sorted(dense))).sum())
    assert lay["nnz_sparse"] == int((~np.isin(a["col"], lay["hot_ids"])).sum())
    # scoring
    yh = fm.predict(ds)
    oy = oracle.predict(a["w0"], a["w"], a["v"], a["row_ptr"], a["col"], a["val"])
    assert (np.abs(yh - oy) <= TOL_Y * term_scale(a)).all()
    assert fm.computeRMSE(ds) == pytest.approx(oracle.rmse(a["w0"], a["w"], a["v"], a["row_ptr"], a["col"], a["val"], a["y"]), rel=1e-5)
    # transposes: the caller sees every feature, hot or not, bit-exact
    for j in range(ds.n_batches):
        lo, hi = j * br, min(n_rows, (j + 1) * br)
        sub = a["row_ptr"][lo:hi + 1] - a["row_ptr"][lo]
        sl = slice(a["row_ptr"][lo], a["row_ptr"][hi])
        cp, rows, cv = oracle.transpose(a["n1"], sub, a["col"][sl], a["val"][sl])
        feat, ptr, drows, dvals = ds.transposeInput(j)
        present = np.nonzero(np.diff(cp))[0]
        np.testing.assert_array_equal(feat, present.astype(np.int32))
        np.testing.assert_array_equal(ptr, cp[np.r_[present, a["n1"]]].astype(np.int32))
        np.testing.assert_array_equal(drows, rows)
        np.testing.assert_array_equal(dvals.astype(np.float64), cv)
    # gradient of every batch, and its run-to-run identity
    for j in range(ds.n_batches):
        lo, hi = j * br, min(n_rows, (j + 1) * br)
        gv, gw, g0, st = fm.batchGradient(ds, j)
        ogv, ogw, og0, osse, _ = oracle.batch_grad(a["w0"], a["w"], a["v"], lo, hi, a["row_ptr"], a["col"], a["val"], a["y"],
                                                   threads=4)
        check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
        assert st["nnz"] == a["row_ptr"][hi] - a["row_ptr"][lo]
        gv2, gw2, _, _ = fm.batchGradient(ds, j)
        np.testing.assert_array_equal(gv, gv2)
        np.testing.assert_array_equal(gw, gw2)
    # training
    eta, regs = 0.02, (0.0, 1e-3, 1e-3)
    sgd = fmhip.HipSGD(eta=eta, reg0=regs[0], regw=regs[1], regv=regs[2])
    w0, w, v = a["w0"], a["w"], a["v"]
    for _ in range(3):
        fm = sgd.learn(fm, ds)
        w0, w, v, sse = oracle.sgd_epoch(w0, w, v, br, a["row_ptr"], a["col"], a["val"], a["y"], eta, *regs)
        assert sgd.last_stats["sse"] == pytest.approx(sse, rel=1e-5)
    assert np.linalg.norm(fm.v - v) <= 1e-4 * np.linalg.norm(v)
    assert np.linalg.norm(fm.w - w) <= 1e-4 * np.linalg.norm(w)
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("k,n_hot,n_low", [(32, 30, 27), (64, 12, 10), (16, 40, 39), (256, 30, 27)])
def test_dense_hot_block_with_a_thin_first_page(fmhip, k, n_hot, n_low):
    """Few features pass the 10 % mark of the two-sided page, many the 5 % mark of the gradient-side pages: page 0 is
    partly (or, with a single 10 % feature, not at all: then there is no hot block) filled, the others follow behind its
    unused slots.  Layout, predictions, every batch's gradient, bit-exact transposes, two epochs."""
    a, hot_ids = hot_problem(300 + k, 4000, 600, k, n_hot, n_low=n_low)
    a["val"] = a["val"].astype(np.float32).astype(np.float64)
    n_rows, br = 4000, 900
    ds, fm = make(fmhip, a, batch_rows=br)
    lay = ds.layout()
    if n_hot - n_low < 2:
        assert lay["hot_pages"] == 0 and lay["hot_ids_all"] == [] and lay["nnz_sparse_backward"] == len(a["col"])
    else:
        assert sorted(lay["hot_ids"]) == sorted(int(x) for x in hot_ids[:n_hot - n_low])
        assert sorted(lay["hot_ids_all"]) == sorted(int(x) for x in hot_ids) and lay["hot_pages"] == 1 + (n_low + 15) // 16
    yh = fm.predict(ds)
    oy = oracle.predict(a["w0"], a["w"], a["v"], a["row_ptr"], a["col"], a["val"])
    assert (np.abs(yh - oy) <= TOL_Y * term_scale(a)).all()
    for j in range(ds.n_batches):
        lo, hi = j * br, min(n_rows, (j + 1) * br)
        gv, gw, g0, st = fm.batchGradient(ds, j)
        ogv, ogw, og0, osse, _ = oracle.batch_grad(a["w0"], a["w"], a["v"], lo, hi, a["row_ptr"], a["col"], a["val"], a["y"], threads=4)
        check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
        sub = a["row_ptr"][lo:hi + 1] - a["row_ptr"][lo]
        sl = slice(a["row_ptr"][lo], a["row_ptr"][hi])
        cp, rows, cv = oracle.transpose(a["n1"], sub, a["col"][sl], a["val"][sl])
        feat, ptr, drows, dvals = ds.transposeInput(j)
        present = np.nonzero(np.diff(cp))[0]
        np.testing.assert_array_equal(feat, present.astype(np.int32))
        np.testing.assert_array_equal(drows, rows)
        np.testing.assert_array_equal(dvals.astype(np.float64), cv)
    eta, regs = 0.02, (0.0, 1e-3, 1e-3)
    sgd = fmhip.HipSGD(eta=eta, reg0=regs[0], regw=regs[1], regv=regs[2])
    w0, w, v = a["w0"], a["w"], a["v"]
    for _ in range(2):
        fm = sgd.learn(fm, ds)
        w0, w, v, sse = oracle.sgd_epoch(w0, w, v, br, a["row_ptr"], a["col"], a["val"], a["y"], eta, *regs)
        assert sgd.last_stats["sse"] == pytest.approx(sse, rel=1e-5)
    assert np.linalg.norm(fm.v - v) <= 1e-4 * np.linalg.norm(v) and np.linalg.norm(fm.w - w) <= 1e-4 * np.linalg.norm(w)
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("k", [4, 32])
def test_dense_hot_block_takes_every_feature(fmhip, k):
    """A dataset whose every feature is frequent (10 features, each in roughly half of the rows): the
    sparse streams of its batches are EMPTY and the whole step runs through the dense block."""
    rng = np.random.default_rng(17 + k)
    n_rows, n1 = 900, 10
    rows = [np.sort(rng.choice(n1, size=int(rng.integers(1, 9)), replace=False)).astype(np.int32) for _ in range(n_rows)]
    rows[5] = np.zeros(0, np.int32)                                  # and an empty row
    row_ptr = np.zeros(n_rows + 1, np.int64)
    row_ptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate(rows)
    a = dict(k=k, n1=n1, w0=0.1, w=rng.normal(0, 0.2, n1), v=rng.normal(0, 0.2, (k, n1)), row_ptr=row_ptr, col=col,
             val=rng.uniform(0.2, 1.5, len(col)), y=rng.normal(0, 1, n_rows))
    ds, fm = make(fmhip, a, batch_rows=250)
    yh = fm.predict(ds)
    oy = oracle.predict(a["w0"], a["w"], a["v"], row_ptr, col, a["val"])
    assert (np.abs(yh - oy) <= TOL_Y * term_scale(a)).all()
    for j in range(ds.n_batches):
        lo, hi = j * 250, min(n_rows, (j + 1) * 250)
        bi = ds.batch_info(j)
        assert bi["nnz"] == row_ptr[hi] - row_ptr[lo] and bi["n_columns"] == len(np.unique(col[row_ptr[lo]:row_ptr[hi]]))
        gv, gw, g0, st = fm.batchGradient(ds, j)
        ogv, ogw, og0, osse, _ = oracle.batch_grad(a["w0"], a["w"], a["v"], lo, hi, row_ptr, col, a["val"], a["y"])
        check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
        feat, ptr, trows, tvals = ds.transposeInput(j)
        assert ptr[-1] == bi["nnz"] and len(feat) == bi["n_columns"]
    eta, regs = 0.05, (0.01, 1e-3, 1e-3)
    sgd = fmhip.HipSGD(eta=eta, reg0=regs[0], regw=regs[1], regv=regs[2])
    w0, w, v = a["w0"], a["w"], a["v"]
    for _ in range(4):
        fm = sgd.learn(fm, ds)
        w0, w, v, sse = oracle.sgd_epoch(w0, w, v, 250, row_ptr, col, a["val"], a["y"], eta, *regs)
        assert sgd.last_stats["sse"] == pytest.approx(sse, rel=1e-5)
    assert np.linalg.norm(fm.v - v) <= 1e-4 * np.linalg.norm(v)
    assert np.linalg.norm(fm.w - w) <= 1e-4 * np.linalg.norm(w)
    ds.unpersist()
    fm.close()


def test_dense_hot_block_chunked_backward(fmhip):
    """The feature-interval backward on a dataset with a dense hot block: the hot rows are complete
    after the first interval's call, whatever interval their ids fall into."""
    import ctypes as C
    from sparkfm_amd import _ffi
    L = _ffi.load()
    a, hot_ids = hot_problem(77, 2500, 600, 32, 14)
    try:
        L.fmhip_tune(_ffi.TUNE_HOT_BLOCK, 1)
        ds, fm = make(fmhip, a, batch_rows=900, stream=torch_stream())
    finally:
        L.fmhip_tune(_ffi.TUNE_HOT_BLOCK, 1)
    import torch
    from sparkfm_amd.distributed import HipEngine
    eng = HipEngine(fm, ds)
    for batch in range(ds.n_batches):
        eng.compute(batch)
        torch.cuda.synchronize()
        want = eng.grad.clone()
        eng.grad.zero_()
        torch.cuda.synchronize()
        _ffi.check(L.fmhip_grad_bind(fm.handle, C.c_void_p(eng.grad.data_ptr())))   # marks the zeroed buffer clean
        for cuts in ([0, 600], [0, 37, 300, 301, 600], [0, int(hot_ids[3]), int(hot_ids[3]) + 1, 600]):
            for ascending in (False, True):      # ascending: the hot rows ride in the FIRST call (it starts at feature 0)
                eng.forward(batch)
                for i in (range(1, len(cuts)) if ascending else range(len(cuts) - 1, 0, -1)):
                    eng.backward(batch, cuts[i - 1], cuts[i], finish=(i == 1))
                torch.cuda.synchronize()
                assert torch.equal(eng.grad, want), (cuts, ascending)
                eng.grad.zero_()
                torch.cuda.synchronize()
                _ffi.check(L.fmhip_grad_bind(fm.handle, C.c_void_p(eng.grad.data_ptr())))
    eng.close()
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("k,hot", [(32, 1), (32, 0), (64, 1), (16, 1), (256, 1), (200, 0)])
def test_band_affine_placement_of_the_backward(fmhip, request, k, hot):
    """fmhip_model_tune(m, _ffi.TUNE_XCD_PLACEMENT, 2): the whole-batch backward takes its ranges from per-XCD lists — the ranges of long columns
    that fall into an XCD's own row bands first (fmhip_dataset.hip: plan_bands) — and forms no wave sums.  Which slot walks a
    range changes nothing about what the range contributes: the gradient must agree with the default placement (to the
    summation order of the cut columns' partials) and with the oracle, run to run bit-identical, and training must track
    the oracle.  Batches of ~200k transposed entries (3,000 ranges: the plan exists from 1,024 on), Zipf ids so that some
    columns span hundreds of ranges, with and without the dense hot block."""
    from sparkfm_amd import _ffi, synth
    L = _ffi.load()
    L.fmhip_tune(_ffi.TUNE_HOT_BLOCK, hot)
    request.addfinalizer(lambda: L.fmhip_tune(_ffi.TUNE_HOT_BLOCK, 1))
    d = synth.make_zipf(4100 + k, 40_000, 3000, 10, 30, zipf_s=1.05)
    rng = np.random.default_rng(k)
    a = dict(n1=3000, k=k, row_ptr=d["row_ptr"], col=d["col"], val=d["val"].astype(np.float64), y=d["y"].astype(np.float64),
             w0=0.1, w=rng.normal(0, 0.05, 3000), v=rng.normal(0, 0.05, (k, 3000)))
    br = 20_000
    ds, fm = make(fmhip, a, batch_rows=br)
    lay = ds.layout()
    assert lay["planned_ranges"] == lay["ranges"] > 2048 and 0 < lay["band_affine_ranges"] < lay["ranges"]
    grads = {}
    for mode in (0, 2, 2):
        _ffi.check(L.fmhip_model_tune(fm.handle, _ffi.TUNE_XCD_PLACEMENT, mode))
        grads.setdefault(mode, []).append(fm.batchGradient(ds, 1))
    (gv0, gw0, g00, st0), = grads[0]
    (gv2, gw2, g02, st2), (gv2b, gw2b, _, _) = grads[2]
    np.testing.assert_array_equal(gv2, gv2b)                      # deterministic
    np.testing.assert_array_equal(gw2, gw2b)
    assert st0["nnz"] == st2["nnz"] and g00 == g02
    ogv, ogw, og0, osse, _ = oracle.batch_grad(a["w0"], a["w"], a["v"], br, 2 * br, a["row_ptr"], a["col"], a["val"], a["y"], threads=8)
    check_grad(gv2, gw2, ogv, ogw, np.abs(a["v"]).max())
    check_grad(gv2, gw2, gv0, gw0, np.abs(a["v"]).max())
    # training with the placement on: the fused step (merged finish / rows-only update) must take it too
    eta, regs = 0.02, (0.0, 1e-3, 1e-3)
    sgd = fmhip.HipSGD(eta=eta, reg0=regs[0], regw=regs[1], regv=regs[2])
    w0, w, v = a["w0"], a["w"], a["v"]
    for _ in range(2):
        fm = sgd.learn(fm, ds)
        w0, w, v, sse = oracle.sgd_epoch(w0, w, v, br, a["row_ptr"], a["col"], a["val"], a["y"], eta, *regs, threads=8)
        assert sgd.last_stats["sse"] == pytest.approx(sse, rel=1e-5)
    assert np.linalg.norm(fm.v - v) <= 1e-4 * np.linalg.norm(v) and np.linalg.norm(fm.w - w) <= 1e-4 * np.linalg.norm(w)
    ds.unpersist()
    fm.close()


def test_band_affine_placement_with_feature_intervals(fmhip):
    """The feature-interval launches of the data-parallel step take their ranges from the same per-XCD lists — each run
    of a list cut down to the launch's range window: fmhip_step_forward + fmhip_step_backward over descending intervals
    must fill the packed gradient exactly like the whole-batch backward (bit for bit: the same partials, the same order),
    for cuts inside hot columns, at column starts, around empty intervals and with the dense hot block on."""
    import ctypes as C
    import torch
    from sparkfm_amd import _ffi, synth
    from sparkfm_amd.distributed import HipEngine
    L = _ffi.load()
    d = synth.make_zipf(4300, 40_000, 3000, 10, 30, zipf_s=1.05)
    rng = np.random.default_rng(3)
    a = dict(n1=3000, k=32, row_ptr=d["row_ptr"], col=d["col"], val=d["val"].astype(np.float64), y=d["y"].astype(np.float64),
             w0=0.1, w=rng.normal(0, 0.05, 3000), v=rng.normal(0, 0.05, (32, 3000)))
    ds, fm = make(fmhip, a, batch_rows=20_000, stream=torch_stream())
    lay = ds.layout()
    assert lay["planned_ranges"] == lay["ranges"] > 2048 and 0 < lay["band_affine_ranges"] < lay["ranges"]
    eng = HipEngine(fm, ds)
    eng.compute(1)
    torch.cuda.synchronize()
    want = eng.grad.clone()
    ogv, ogw, og0, osse, _ = oracle.batch_grad(a["w0"], a["w"], a["v"], 20_000, 40_000, a["row_ptr"], a["col"], a["val"], a["y"], threads=8)
    gv, gw, _, _ = fm.batchGradient(ds, 1)
    check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
    eng.grad.zero_()
    torch.cuda.synchronize()
    fm_h = fm.handle
    _ffi.check(L.fmhip_grad_bind(fm_h, C.c_void_p(eng.grad.data_ptr())))
    for cuts in ([0, 3000], [0, 70, 3000], [0, 3, 64, 65, 700, 2999, 3000], [0, 1500, 1500, 3000]):
        for ascending in (False, True):
            eng.forward(1)
            for i in (range(1, len(cuts)) if ascending else range(len(cuts) - 1, 0, -1)):
                eng.backward(1, cuts[i - 1], cuts[i], finish=(i == 1))
            torch.cuda.synchronize()
            assert torch.equal(eng.grad, want), (cuts, ascending)
            eng.grad.zero_()
            torch.cuda.synchronize()
            _ffi.check(L.fmhip_grad_bind(fm_h, C.c_void_p(eng.grad.data_ptr())))
    eng.close()
    ds.unpersist()
    fm.close()


def test_transpose_is_bit_exact(fmhip):
    """The device-resident per-batch transposes (S/DataSet.scala:31-38) against the oracle's:
    feature ids, row ids and values must match exactly (index gathers are bit-exact)."""
    a = random_problem(5, 700, 90, 4, 0, 25, empty_rows=(5,))
    a["val"] = a["val"].astype(np.float32).astype(np.float64)       # exactly representable in fp32
    ds, fm = make(fmhip, a, batch_rows=256)
    for b in range(3):
        r0, r1 = b * 256, min(700, (b + 1) * 256)
        sub = a["row_ptr"][r0:r1 + 1] - a["row_ptr"][r0]
        sl = slice(a["row_ptr"][r0], a["row_ptr"][r1])
        cp, rows, cv = oracle.transpose(a["n1"], sub, a["col"][sl], a["val"][sl])
        feat, ptr, drows, dvals = ds.transposeInput(b)
        present = np.nonzero(np.diff(cp))[0]
        np.testing.assert_array_equal(feat, present.astype(np.int32))
        np.testing.assert_array_equal(ptr, cp[np.r_[present, a["n1"]]].astype(np.int32) if len(present) else [0])
        np.testing.assert_array_equal(drows, rows)
        np.testing.assert_array_equal(dvals.astype(np.float64), cv)
    ds.unpersist()
    fm.close()


def test_single_nonzero_rows_have_exactly_zero_interaction(fmhip):
    a = random_problem(9, 500, 64, 32, 1, 1)
    ds, fm = make(fmhip, a)
    yh = fm.predict(ds).astype(np.float32)
    w32, x32 = a["w"].astype(np.float32), a["val"].astype(np.float32)
    lin = np.float32(a["w0"]) + w32[a["col"]] * x32                 # one fp32 product + one add
    np.testing.assert_array_equal(yh, lin.astype(np.float32))
    gv, gw, g0, st = fm.batchGradient(ds, 0)
    assert np.abs(gv).max() <= 1e-6 * np.abs(a["v"]).max() * np.abs(gw).max()   # h(v) = x*(v x) - x^2 v = 0 (to fp32 rounding)
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("k,flat", [(16, 0), (32, 0), (32, 1), (64, 0), (100, 0), (127, 1), (200, 0), (200, 1), (256, 0), (256, 1)])
def test_row_lengths_around_the_step_boundaries(fmhip, k, flat):
    """The forward walks a row 8 (k <= 64) or 16 entries per step; through a buffer view the row's last, partial step is a
    full step whose dead entries are id -1 with value 0, and the next step's entries are requested a step ahead; flat
    addresses (forced here with tuning key 8) keep the masked last step.  Rows of every length 0..40 — each boundary from
    both sides, several times over, in a persistent grid that gives a slot more than one row — predict like the oracle,
    and the one-entry rows are exactly linear (quirk Q6)."""
    rng = np.random.default_rng(40 + k)
    n_rows, n1 = 41 * 60, 300
    lens = np.tile(np.arange(41), 60)
    rng.shuffle(lens)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    col = np.concatenate([rng.choice(n1, size=n, replace=False) for n in lens]).astype(np.int32)
    val = np.where(rng.random(len(col)) < 0.5, 1.0, rng.uniform(0.1, 1.0, len(col)))
    a = dict(k=k, n1=n1, w0=0.3, w=rng.normal(0, 0.1, n1), v=rng.normal(0, 0.1, (k, n1)), row_ptr=row_ptr, col=col, val=val,
             y=rng.normal(0, 1.0, n_rows))
    from sparkfm_amd import _ffi
    L = _ffi.load()
    if flat:
        L.fmhip_tune(_ffi.TUNE_FLAT_ADDRESS, 1)
    try:
        ds, fm = make(fmhip, a, batch_rows=1300)               # two batches: the dense hot block may form, too
        yh = fm.predict(ds)
        oyh = oracle.predict(a["w0"], a["w"], a["v"], row_ptr, col, val)
        assert (np.abs(yh - oyh) <= TOL_Y * term_scale(a)).all()
        assert (yh[lens == 0] == np.float32(0.3)).all()
        one = np.flatnonzero(lens == 1)
        lin = np.float32(0.3) + a["w"].astype(np.float32)[col[row_ptr[one]]] * val[row_ptr[one]].astype(np.float32)
        np.testing.assert_array_equal(yh[one].astype(np.float32), lin.astype(np.float32))
        gv, gw, g0, st = fm.batchGradient(ds, 1)
        ogv, ogw, og0, osse, oe = oracle.batch_grad(a["w0"], a["w"], a["v"], 1300, n_rows, row_ptr, col, val, a["y"])
        check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
        assert st["sse"] == pytest.approx(osse, rel=1e-5) and st["rows"] == n_rows - 1300
        ds.unpersist()
        fm.close()
    finally:
        if flat:
            L.fmhip_tune(_ffi.TUNE_FLAT_ADDRESS, 0)


def test_hot_columns_split_over_many_ranges(fmhip):
    """Power-law columns: 3 features present in every row (columns of 4000 entries = 63 ranges
    each) next to a long tail of 1-2 entry columns."""
    rng = np.random.default_rng(77)
    n_rows, n1, k = 4000, 3000, 32
    rows = []
    for r in range(n_rows):
        tail = rng.choice(np.arange(3, n1), size=int(rng.integers(0, 4)), replace=False)
        idx = np.concatenate([rng.permutation(3), tail]).astype(np.int32)
        rows.append(idx)
    row_ptr = np.zeros(n_rows + 1, np.int64)
    row_ptr[1:] = np.cumsum([len(r) for r in rows])
    col = np.concatenate(rows)
    val = rng.uniform(0.1, 1.0, len(col))
    a = dict(k=k, n1=n1, w0=0.3, w=rng.normal(0, 0.1, n1), v=rng.normal(0, 0.1, (k, n1)), row_ptr=row_ptr, col=col,
             val=val, y=rng.normal(0, 1, n_rows))
    ds, fm = make(fmhip, a)
    gv, gw, g0, st = fm.batchGradient(ds, 0)
    ogv, ogw, og0, osse, _ = oracle.batch_grad(a["w0"], a["w"], a["v"], 0, n_rows, row_ptr, col, val, a["y"], threads=4)
    check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
    gv2, gw2, _, _ = fm.batchGradient(ds, 0)
    np.testing.assert_array_equal(gv, gv2)                          # atomics-free: run-to-run identical
    np.testing.assert_array_equal(gw, gw2)
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("k", [4, 16, 32, 64, 129, 256])
def test_column_lengths_around_the_range_and_wave_boundaries(fmhip, k):
    """Columns of every length 1..700 (ranges are 64 entries, a slot finishes a column that ends
    <= 16 entries behind its range, a wave sums 64/LPN ranges when they lie in one column): every
    combination of direct store / head / tail / wave partial occurs."""
    rng = np.random.default_rng(5 + k)
    n_rows, lens = 800, list(range(1, 701, 3)) + [64, 65, 80, 81, 128, 512, 513, 640, 800]
    rng.shuffle(lens)
    n1 = len(lens)
    cols = [np.sort(rng.choice(n_rows, size=ln, replace=False)) for ln in lens]
    rr = np.concatenate(cols)
    cc = np.concatenate([np.full(len(c), j, np.int32) for j, c in enumerate(cols)])
    order = np.lexsort((rng.random(len(rr)), rr))                    # by row, random order inside a row
    rr, cc = rr[order], cc[order]
    row_ptr = np.zeros(n_rows + 1, np.int64)
    np.add.at(row_ptr, rr + 1, 1)
    row_ptr = np.cumsum(row_ptr)
    a = dict(k=k, n1=n1, w0=-0.2, w=rng.normal(0, 0.1, n1), v=rng.normal(0, 0.05, (k, n1)), row_ptr=row_ptr,
             col=cc.astype(np.int32), val=rng.uniform(0.1, 1.0, len(cc)), y=rng.normal(0, 1, n_rows))
    ds, fm = make(fmhip, a)
    gv, gw, g0, st = fm.batchGradient(ds, 0)
    ogv, ogw, og0, osse, _ = oracle.batch_grad(a["w0"], a["w"], a["v"], 0, n_rows, row_ptr, a["col"], a["val"], a["y"],
                                               threads=4)
    check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
    gv2, gw2, _, _ = fm.batchGradient(ds, 0)
    np.testing.assert_array_equal(gv, gv2)
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("k,batch_rows", [(8, 128), (32, 500), (64, 2000)])
def test_sgd_epochs_track_the_oracle(fmhip, k, batch_rows):
    a = random_problem(40 + k, 2000, 400, k, 1, 30)
    rng = np.random.default_rng(1)
    vt = rng.normal(0, 0.3, (2, 400))                               # learnable targets: a planted FM
    a["y"] = oracle.predict(0.2, rng.normal(0, 0.3, 400), vt, a["row_ptr"], a["col"], a["val"]) + rng.normal(0, .05, 2000)
    ds, fm = make(fmhip, a, batch_rows=batch_rows)
    eta, regs = 0.05, (0.0, 1e-3, 1e-3)
    sgd = fmhip.HipSGD(eta=eta, reg0=regs[0], regw=regs[1], regv=regs[2])
    w0, w, v = a["w0"], a["w"], a["v"]
    losses_gpu, losses_cpu = [], []
    for _ in range(5):
        fm = sgd.learn(fm, ds)
        w0, w, v, sse = oracle.sgd_epoch(w0, w, v, batch_rows, a["row_ptr"], a["col"], a["val"], a["y"], eta, *regs)
        losses_gpu.append(sgd.last_stats["sse"])
        losses_cpu.append(sse)
    assert sgd.last_stats["rows"] == 2000 and sgd.last_stats["steps"] == -(-2000 // batch_rows)
    np.testing.assert_allclose(losses_gpu, losses_cpu, rtol=1e-5)
    assert losses_cpu[-1] < losses_cpu[0]
    assert np.linalg.norm(fm.v - v) <= 1e-4 * np.linalg.norm(v)
    assert np.linalg.norm(fm.w - w) <= 1e-4 * np.linalg.norm(w)
    assert fm.w0 == pytest.approx(w0, rel=1e-4, abs=1e-6)
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("k", [16, 32, 64, 200, 256])
def test_rows_only_apply_for_wide_models(fmhip, k):
    """Without weight decay a step may update just the rows its batch touched (a model far wider than a
    batch: the dense pass would rewrite every other row unchanged).  Same parameters, bit for bit, as
    the dense update of the split-step path; both track the oracle."""
    import torch
    from sparkfm_amd.distributed import DataParallelSGD
    a, _ = hot_problem(300 + k, 1500, 40000, k, 6)
    ds, fm = make(fmhip, a, batch_rows=400)
    fm2 = fmhip.FMModel(a["n1"] - 1, k, stream=torch_stream())
    fm2.w0, fm2.w, fm2.v = a["w0"], a["w"], a["v"]
    eta = 0.05
    sgd = fmhip.HipSGD(eta=eta, reg0=0.0, regw=0.0, regv=0.0)            # fused path: rows-only apply
    dp = DataParallelSGD(eta=eta, reg0=0.0, regw=0.0, regv=0.0)           # split-step path: dense apply
    w0, w, v = a["w0"], a["w"], a["v"]
    for _ in range(3):
        fm = sgd.learn(fm, ds)
        dp.learn(fm2, ds)
        w0, w, v, sse = oracle.sgd_epoch(w0, w, v, 400, a["row_ptr"], a["col"], a["val"], a["y"], eta, 0.0, 0.0, 0.0)
        assert sgd.last_stats["sse"] == pytest.approx(sse, rel=1e-5)
    torch.cuda.synchronize()
    assert fm.w0 == fm2.w0
    np.testing.assert_array_equal(fm.w, fm2.w)
    np.testing.assert_array_equal(fm.v, fm2.v)
    assert np.linalg.norm(fm.v - v) <= 1e-4 * np.linalg.norm(v)
    assert np.linalg.norm(fm.w - w) <= 1e-4 * max(np.linalg.norm(w), 1e-12)
    untouched = np.setdiff1d(np.arange(a["n1"]), a["col"])
    np.testing.assert_array_equal(fm.v[:, untouched], a["v"][:, untouched].astype(np.float32))
    ds.unpersist()
    fm.close()
    fm2.close()


@pytest.mark.parametrize("k", [2, 8, 32])
def test_rows_only_update_when_every_feature_sits_in_the_hot_block(fmhip, k):
    """A dataset whose every feature is dense enough for the hot block has NO sparse columns (n_cols = 0 in every batch, an
    empty feature list) under a model far wider than the batch touches: the update must still be the rows-only one — the
    decay of the untouched rows rides in the tables' scale exactly once.  (Found by tools/soak_random_shapes.py: the update
    kernel was chosen by `feat != NULL`, an empty list was NULL, the dense pass applied the decay and the host scaled the
    tables as well — every parameter decayed twice, then three times, ...)"""
    rng = np.random.default_rng(5)
    n_rows, n1, feats = 40, 700, rng.choice(700, size=30, replace=False).astype(np.int32)
    row_ptr = np.arange(n_rows + 1, dtype=np.int64) * 30
    col = np.concatenate([rng.permutation(feats) for _ in range(n_rows)]).astype(np.int32)
    val = rng.uniform(0.1, 1.0, len(col))
    a = dict(k=k, n1=n1, w0=0.1, w=rng.normal(0, 0.1, n1), v=rng.normal(0, 0.1, (k, n1)), row_ptr=row_ptr, col=col, val=val,
             y=rng.normal(0, 1.0, n_rows))
    ds, fm = make(fmhip, a, batch_rows=10)
    lay = ds.layout()
    assert len([i for i in lay["hot_ids_all"] if i >= 0]) == 30 and lay["nnz_sparse_backward"] == 0   # all thirty features are in the block: no transposes left
    eta, regs = 0.01, (0.01, 0.01, 0.01)
    fmhip.HipSGD(eta=eta, reg0=regs[0], regw=regs[1], regv=regs[2]).learn(fm, ds)
    w0, w, v, sse = oracle.sgd_epoch(a["w0"], a["w"], a["v"], 10, row_ptr, col, val, a["y"], eta, *regs)
    untouched = np.setdiff1d(np.arange(n1), feats)
    np.testing.assert_allclose(fm.v[:, untouched], a["v"][:, untouched] * (1 - eta * regs[2]) ** 4, rtol=2e-6)   # four steps of decay, once each
    assert np.linalg.norm(fm.v - v) <= 1e-5 * np.linalg.norm(v)
    assert np.linalg.norm(fm.w - w) <= 1e-5 * max(np.linalg.norm(w), 1e-9)
    ds.unpersist()
    fm.close()


def test_batch_order_and_determinism(fmhip):
    a = random_problem(61, 1500, 300, 16, 1, 20)
    outs = []
    for rep in range(2):
        ds, fm = make(fmhip, a, batch_rows=400)
        sgd = fmhip.HipSGD(eta=0.03, regv=1e-3, shuffle_seed=5)
        for _ in range(3):
            fm = sgd.learn(fm, ds)
        outs.append((fm.w0, fm.w.copy(), fm.v.copy()))
        ds.unpersist()
        fm.close()
    assert outs[0][0] == outs[1][0]
    np.testing.assert_array_equal(outs[0][1], outs[1][1])            # bit-identical run to run
    np.testing.assert_array_equal(outs[0][2], outs[1][2])
    # the same permuted schedule on the oracle
    sgd = fmhip.HipSGD(eta=0.03, regv=1e-3, shuffle_seed=5)
    w0, w, v = a["w0"], a["w"], a["v"]
    for _ in range(3):
        order = sgd.batch_order(4)
        sgd._epoch += 1
        w0, w, v, _ = oracle.sgd_epoch(w0, w, v, 400, a["row_ptr"], a["col"], a["val"], a["y"], 0.03, 0, 0, 1e-3,
                                       order=order)
    assert np.linalg.norm(outs[0][2] - v) <= 1e-4 * np.linalg.norm(v)


def test_split_step_equals_fused_step(fmhip):
    """fmhip_step_compute + fmhip_step_apply with a caller-owned (torch) gradient buffer ==
    fmhip_sgd_step; this is the path the data-parallel trainer uses."""
    import torch
    from sparkfm_amd.distributed import DataParallelSGD, HipEngine
    a = random_problem(71, 900, 200, 32, 1, 20)
    ds, fm = make(fmhip, a, batch_rows=300)
    ref = fmhip.HipSGD(eta=0.04, regw=1e-3, regv=1e-3)
    ref.learn(fm, ds)
    want = (fm.w0, fm.w.copy(), fm.v.copy())
    fm2 = fmhip.FMModel(a["n1"] - 1, a["k"], stream=torch_stream())
    fm2.w0, fm2.w, fm2.v = a["w0"], a["w"], a["v"]
    dp = DataParallelSGD(eta=0.04, regw=1e-3, regv=1e-3)
    dp.learn(fm2, ds)
    assert dp.plan_cuts(dp.engine(fm2, ds))[0] == 0 and dp.cuts[-1] == a["n1"]
    torch.cuda.synchronize()
    assert fm2.w0 == want[0]
    np.testing.assert_array_equal(fm2.w, want[1])
    np.testing.assert_array_equal(fm2.v, want[2])
    g = dp.engine(fm2, ds).grad
    assert float(g[32:].abs().max()) == 0.0                          # apply leaves G_w/G_b/G_V zeroed
    assert float(g[2]) == 300.0                                      # scalars keep the last step's {.., rows, ..}
    ds.unpersist()
    fm.close()
    fm2.close()


def test_feature_chunked_backward_equals_whole_backward(fmhip):
    """fmhip_step_forward + fmhip_step_backward over descending feature intervals fills the packed
    gradient exactly like fmhip_step_compute (bit for bit): the overlap path of the data-parallel
    trainer.  Cuts are placed inside ranges, at range boundaries, and around empty intervals."""
    import ctypes as C
    import torch
    from sparkfm_amd import _ffi
    from sparkfm_amd.distributed import HipEngine
    L = _ffi.load()
    a = random_problem(81, 3000, 400, 32, 1, 30)
    for r in range(3000):                                            # two hot columns -> wave sums + long fixups
        s = slice(a["row_ptr"][r], a["row_ptr"][r + 1])
        a["col"][s.start] = 0 if not (a["col"][s] == 0).any() else a["col"][s.start]
    ds, fm = make(fmhip, a, batch_rows=1500, stream=torch_stream())
    eng = HipEngine(fm, ds)
    for batch in (0, 1):
        eng.compute(batch)
        torch.cuda.synchronize()
        want = eng.grad.clone()
        eng.grad.zero_()
        torch.cuda.synchronize()
        fm_h = fm.handle
        _ffi.check(L.fmhip_grad_bind(fm_h, C.c_void_p(eng.grad.data_ptr())))   # marks the zeroed buffer clean
        for cuts in ([0, 400], [0, 1, 400], [0, 7, 50, 51, 399, 400], [0, 200, 200, 400]):
            for ascending in (False, True):      # from the top down, or from feature 0 up (the straddling range goes with the other side)
                eng.forward(batch)
                order = range(1, len(cuts)) if ascending else range(len(cuts) - 1, 0, -1)
                for i in order:
                    eng.backward(batch, cuts[i - 1], cuts[i], finish=(i == 1))
                torch.cuda.synchronize()
                assert torch.equal(eng.grad, want), (cuts, ascending)
                eng.grad.zero_()
                torch.cuda.synchronize()
                _ffi.check(L.fmhip_grad_bind(fm_h, C.c_void_p(eng.grad.data_ptr())))
    # order is enforced: the first interval ends at n+1 or starts at 0, the others follow it
    eng.forward(0)
    assert L.fmhip_step_backward(fm.handle, ds.handle, 0, 50, 100, 0) == -1
    assert b"descending" in L.fmhip_last_error()
    assert L.fmhip_step_backward(fm.handle, ds.handle, 0, 0, 100, 1) == 0          # ascending it is
    assert L.fmhip_step_backward(fm.handle, ds.handle, 0, 200, 401, 0) == -1
    assert b"ascending" in L.fmhip_last_error()
    assert L.fmhip_step_backward(fm.handle, ds.handle, 0, 100, 401, 0) == 0
    torch.cuda.synchronize()
    eng.grad.zero_()
    torch.cuda.synchronize()
    eng.close()
    ds.unpersist()
    fm.close()


def test_errors_are_reported_not_thrown(fmhip):
    from sparkfm_amd import _ffi
    a = random_problem(3, 50, 40, 4, 1, 5)
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"]).cache()
    small = fmhip.FMModel(10, 4)                                     # fewer slots than the data's max index
    with pytest.raises(_ffi.FmhipError) as ei:
        small.computeRMSE(ds)
    assert ei.value.code == -4 and "num_attribute" in str(ei.value)
    with pytest.raises(_ffi.FmhipError):
        fmhip.HipSGD().step(fmhip.FMModel(39, 4), ds, 7)             # batch out of range
    bad = a["col"].copy()
    bad[3] = -1
    with pytest.raises(_ffi.FmhipError):
        fmhip.DataSet(a["row_ptr"], bad, a["val"], a["y"]).cache()
    with pytest.raises(_ffi.FmhipError):
        fmhip.FMModel(10, 1000).handle                               # > FMHIP_MAX_FACTORS
    ds.unpersist()


def test_nonfinite_is_counted_not_masked(fmhip):
    a = random_problem(4, 64, 30, 8, 2, 6)
    a["v"][:, 3] = np.inf
    ds, fm = make(fmhip, a)
    from sparkfm_amd import _ffi
    import ctypes as C
    st = _ffi.Stats()
    r = C.c_double()
    _ffi.check(_ffi.load().fmhip_rmse(fm.handle, ds.handle, C.byref(r), C.byref(st)))
    n_bad = sum(1 for rr in range(64) if (a["col"][a["row_ptr"][rr]:a["row_ptr"][rr + 1]] == 3).any())
    assert st.nonfinite == n_bad and n_bad > 0
    ds.unpersist()
    fm.close()


def test_als_epoch_matches_the_reference_learner(fmhip, kats):
    """fmhip_als_epoch = ALS.learn (S/fm/lib/ALS.scala:15-75) in fp64 on the GPU: against the
    120-digit KATs and against the oracle over several epochs (tree-ordered column sums vs the
    oracle's sequential ones: agreement to fp64 reassociation)."""
    for c in kats:
        a = kat_arrays(c)
        s = c["als"]
        ds, fm = make(fmhip, a)
        fm.reg0, fm.regw, fm.regv = f(s["reg0"]), f(s["regw"]), f(s["regv"])
        fmhip.HipALS.run().learn(fm, ds)
        assert fm.w0 == pytest.approx(f(s["w0"]), rel=1e-10, abs=1e-12)
        np.testing.assert_allclose(fm.w, f(s["w"]), rtol=1e-9, atol=1e-11)
        np.testing.assert_allclose(fm.v, np.array(f(s["V"])), rtol=1e-9, atol=1e-11)
        assert fm.w[-1] == a["w"][-1]                                # quirk Q1: last slot never trained
        np.testing.assert_array_equal(fm.v[:, -1], a["v"][:, -1])
        ds.unpersist()
        fm.close()
    a = random_problem(515, 1500, 120, 6, 0, 14, empty_rows=(7,))
    rng = np.random.default_rng(2)
    a["y"] = oracle.predict(0.3, rng.normal(0, 0.3, 120), rng.normal(0, 0.3, (3, 120)), a["row_ptr"], a["col"],
                            a["val"]) + rng.normal(0, 0.05, 1500)
    ds, fm = make(fmhip, a)
    fm.reg0, fm.regw, fm.regv = 0.0, 0.1, 10.0
    w0, w, v = a["w0"], a["w"], a["v"]
    rm = [fm.computeRMSE(ds)]
    for _ in range(4):
        fmhip.HipALS.run().learn(fm, ds)
        w0, w, v = oracle.als_epoch(w0, w, v, 0.0, 0.1, 10.0, a["row_ptr"], a["col"], a["val"], a["y"])
        rm.append(fm.computeRMSE(ds))
    np.testing.assert_allclose(fm.v, v, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(fm.w, w, rtol=1e-8, atol=1e-11)
    assert fm.w0 == pytest.approx(w0, rel=1e-9)
    assert rm[-1] < 0.5 * rm[0]                                      # ALS converges fast on a planted FM
    assert rm[-1] == pytest.approx(oracle.rmse(w0, w, v, a["row_ptr"], a["col"], a["val"], a["y"]), rel=1e-5)
    # SGD then ALS: the fp64 masters are refreshed from the fp32 device state first
    fmhip.HipSGD(eta=0.01).learn(fm, ds)
    w0, w, v = fm.w0, fm.w.copy(), fm.v.copy()
    fmhip.HipALS.run().learn(fm, ds)
    w0, w, v = oracle.als_epoch(w0, w, v, 0.0, 0.1, 10.0, a["row_ptr"], a["col"], a["val"], a["y"])
    np.testing.assert_allclose(fm.v, v, rtol=1e-8, atol=1e-11)
    multi = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=500).cache()
    from sparkfm_amd import _ffi
    with pytest.raises(_ffi.FmhipError) as ei:
        fmhip.HipALS.run().learn(fm, multi)
    assert ei.value.code == -5
    multi.unpersist()
    ds.unpersist()
    fm.close()


def test_config_c1_fit_with_als(fmhip):
    """BASELINE config 1 — SparkFM fit() on 10k rows x 1k features, k=8 — through the reference's call
    shape FM(dataset, numFactor, maxIteration).learnWith(ALS.run) (S/driver.scala:106-110), on the GPU."""
    from sparkfm_amd import synth
    d = synth.make_config("C1")
    ds = fmhip.DataSet.from_arrays(d, name="C1")                      # single batch: ALS needs the whole transpose
    trainer = fmhip.FM(ds, d["k"], maxIteration=3, seed=5)
    fm = trainer.learnWith(fmhip.HipALS.run())
    w0, w, v = 0.0, np.zeros(ds.dimension + 1), fmhip.FMModel(ds.dimension, 8, seed=5).v
    val, y = d["val"].astype(np.float64), d["y"].astype(np.float64)
    hist = []
    for _ in range(3):
        hist.append(oracle.rmse(w0, w, v, d["row_ptr"], d["col"], val, y))
        w0, w, v = oracle.als_epoch(w0, w, v, 0.0, 0.0, 10.0, d["row_ptr"], d["col"], val, y)
    np.testing.assert_allclose(trainer.rmse_history, hist, rtol=1e-5)
    np.testing.assert_allclose(fm.v, v, rtol=1e-8, atol=1e-12)
    np.testing.assert_allclose(fm.w, w, rtol=1e-8, atol=1e-12)
    assert fm.computeMAE(ds) > 0 and 0.0 <= fm.computeAccuracy(ds) <= 1.0
    assert abs(fm.computeMeanError(ds)) < fm.computeMAE(ds)


@pytest.mark.parametrize("config", ["C3", "C2"])
def test_full_size_properties(fmhip, config):
    """BASELINE configs 3 (k=32, the bench workload) and 2 (k=16: packed rows) at their full size (1M
    rows x 100k features, 40M nonzeros): (1) the oracle on a random sample of rows scored against the full
    model, (2) the FULL gradient of a 250k-row batch (10M nonzeros) element by element against the
    multi-threaded oracle, plus size-independent identities computed outside the backward, (3) bit-identical
    repeats and chunked == whole backward, (4) the dense-hot-block and plain layouts agreeing with each
    other and with the oracle."""
    import ctypes as C
    import torch
    from sparkfm_amd import _ffi, synth
    from sparkfm_amd.distributed import HipEngine
    L = _ffi.load()
    d = synth.make_config(config)
    n_rows, n1, k, br = len(d["row_ptr"]) - 1, synth.CONFIGS[config]["features"], synth.CONFIGS[config]["k"], 250000
    rng = np.random.default_rng(3)
    w0, w, v = 0.05, rng.normal(0, 0.05, n1), rng.normal(0, 0.05, (k, n1))
    row_ptr, col = d["row_ptr"], d["col"]
    val, y = d["val"].astype(np.float64), d["y"].astype(np.float64)

    def build(hot):
        try:
            L.fmhip_tune(_ffi.TUNE_HOT_BLOCK, hot)
            ds = fmhip.DataSet.from_arrays(d, batch_rows=br).cache()
        finally:
            L.fmhip_tune(_ffi.TUNE_HOT_BLOCK, 1)
        fm = fmhip.FMModel(n1 - 1, k, stream=torch_stream())
        fm.w0, fm.w, fm.v = w0, w, v
        return ds, fm

    ds, fm = build(1)
    # (1) the oracle on 3000 sampled rows, full model
    rows = np.sort(rng.choice(n_rows, 3000, replace=False))
    lens = (row_ptr[rows + 1] - row_ptr[rows]).astype(np.int64)
    sub_ptr = np.concatenate([[0], np.cumsum(lens)])
    idx = np.concatenate([np.arange(row_ptr[r], row_ptr[r + 1]) for r in rows])
    oy = oracle.predict(w0, w, v, sub_ptr, col[idx], val[idx])
    yh = fm.predict(ds)
    scale = term_scale(dict(y=oy, row_ptr=sub_ptr, col=col[idx], val=val[idx], w0=w0, w=w, v=v))
    assert (np.abs(yh[rows] - oy) <= TOL_Y * scale).all()
    # (2) identities of batch 0's gradient, from quantities computed independently of the backward
    gv, gw, g0, st = fm.batchGradient(ds, 0)
    e = (yh[:br] - y[:br])                                             # fp32 predictions, fp64 arithmetic from here on
    p0, p1 = row_ptr[0], row_ptr[br]
    assert st["nnz"] == p1 - p0 and st["rows"] == br
    xs = val[p0:p1]
    row_of = np.repeat(np.arange(br), np.diff(row_ptr[:br + 1]))
    assert g0 == pytest.approx(e.sum(), rel=1e-4, abs=1e-3)            # h(w0) = 1
    assert st["sse"] == pytest.approx((e * e).sum(), rel=1e-4)
    ex = e[row_of] * xs
    want_gw = np.bincount(col[p0:p1], weights=ex, minlength=n1)        # G_w[i] = sum_r e_r x_ri, an independent scatter
    np.testing.assert_allclose(gw, want_gw, rtol=2e-4, atol=2e-4 * np.abs(want_gw).max())
    lin = np.bincount(row_of, weights=w[col[p0:p1]] * xs, minlength=br)
    inter = yh[:br] - w0 - lin                                         # 0.5 * sum_f (q_f^2 - s_f)
    # Euler: the interaction is homogeneous of degree 2 in V, so sum_i <v_i, dL/dv_i> = sum_r e_r * 2 * inter_r
    assert float((gv * v).sum()) == pytest.approx(float((e * 2.0 * inter).sum()), rel=2e-3, abs=1e-2)
    # ... and every element of G_V / G_w against the oracle's gradient of the same batch
    ogv, ogw, og0, osse, _ = oracle.batch_grad(w0, w, v, 0, br, row_ptr, col, val, y, threads=min(oracle.max_threads(), 16))
    check_grad(gv, gw, ogv, ogw, np.abs(v).max())
    assert g0 == pytest.approx(og0, rel=1e-4, abs=1e-2) and st["sse"] == pytest.approx(osse, rel=1e-5)
    # (3) determinism and chunked == whole, bit for bit
    gv2, gw2, _, _ = fm.batchGradient(ds, 0)
    np.testing.assert_array_equal(gv, gv2)
    np.testing.assert_array_equal(gw, gw2)
    eng = HipEngine(fm, ds)
    eng.compute(1)
    torch.cuda.synchronize()
    want = eng.grad.clone()
    eng.grad.zero_()
    torch.cuda.synchronize()
    _ffi.check(L.fmhip_grad_bind(fm.handle, C.c_void_p(eng.grad.data_ptr())))
    eng.forward(1)
    cuts = [0, 700, 20000, n1]
    for i in range(len(cuts) - 1, 0, -1):
        eng.backward(1, cuts[i - 1], cuts[i], finish=(i == 1))
    torch.cuda.synchronize()
    assert torch.equal(eng.grad, want)
    eng.close()
    # (4) the layout without the dense hot block computes the same gradient (different summation order only)
    ds_p, fm_p = build(0)
    gv_p, gw_p, g0_p, st_p = fm_p.batchGradient(ds_p, 0)
    check_grad(gv, gw, gv_p, gw_p, np.abs(v).max())
    check_grad(gv_p, gw_p, ogv, ogw, np.abs(v).max())
    assert st_p["sse"] == pytest.approx(st["sse"], rel=1e-6)
    # (5) two SGD steps with weight decay at this size against the oracle's (the steps were compared layout
    # against layout only): the fused step of batches 0 and 1 — the merged finish at these widths — on a fresh model
    thr = min(oracle.max_threads(), 16)
    regs = (0.0, 1e-3, 2e-3)
    o0, ow, ov, _ = oracle.sgd_step(w0, w, v, 0, br, row_ptr, col, val, y, 0.05, *regs, threads=thr)
    o0, ow, ov, osse1 = oracle.sgd_step(o0, ow, ov, br, 2 * br, row_ptr, col, val, y, 0.05, *regs, threads=thr)
    fm_s = fmhip.FMModel(n1 - 1, k)
    fm_s.w0, fm_s.w, fm_s.v = w0, w, v
    st1 = _ffi.Stats()
    _ffi.check(L.fmhip_sgd_step(fm_s.handle, ds.handle, 0, 0.05, *regs, None))
    _ffi.check(L.fmhip_sgd_step(fm_s.handle, ds.handle, 1, 0.05, *regs, C.byref(st1)))
    fm_s._device_updated()
    assert st1.sse == pytest.approx(osse1, rel=1e-5) and st1.rows == br
    assert np.linalg.norm(fm_s.v - ov) <= 1e-5 * np.linalg.norm(ov) and np.linalg.norm(fm_s.w - ow) <= 1e-5 * np.linalg.norm(ow)
    assert np.abs(fm_s.v - ov).max() <= 1e-6 + 1e-5 * np.abs(ov).max() and fm_s.w0 == pytest.approx(o0, rel=1e-5, abs=1e-7)
    fm_s.close()
    # and training moves the loss the same way on both
    for m_, d_ in ((fm, ds), (fm_p, ds_p)):
        fmhip.HipSGD(eta=0.02, regw=1e-4, regv=1e-4).learn(m_, d_)
    r_hot, r_plain = fm.computeRMSE(ds), fm_p.computeRMSE(ds_p)
    assert r_hot == pytest.approx(r_plain, rel=1e-5) and r_hot < math.sqrt(st["sse"] / br)
    for o in (ds, ds_p):
        o.unpersist()
    fm.close()
    fm_p.close()


def test_fit_loop_like_the_reference(fmhip):
    """FM(dataset, numFactor, maxIteration).learnWith(learner) — S/fm/impl/FactorizationMachines.scala:30-51."""
    from sparkfm_amd import synth
    d = synth.make_config("C1")                                      # 10k rows, 1k features, k=8 (BASELINE config 1)
    ds = fmhip.DataSet.from_arrays(d, name="C1", batch_rows=1000)
    trainer = fmhip.FM(ds, d["k"], maxIteration=6, seed=3)
    fm = trainer.learnWith(fmhip.HipSGD.run(eta=0.1, regw=1e-4, regv=1e-4))
    assert fm.num_attribute == ds.dimension and fm.v.shape == (8, ds.dimension + 1)
    assert len(trainer.rmse_history) == 6
    assert trainer.rmse_history[-1] < trainer.rmse_history[0]        # it learns
    # the oracle follows the same trajectory from the same injected start
    w0, w, v = 0.0, np.zeros(ds.dimension + 1), fmhip.FMModel(ds.dimension, 8, seed=3).v
    val, y = d["val"].astype(np.float64), d["y"].astype(np.float64)
    hist = []
    for _ in range(6):
        hist.append(oracle.rmse(w0, w, v, d["row_ptr"], d["col"], val, y))
        w0, w, v, _ = oracle.sgd_epoch(w0, w, v, 1000, d["row_ptr"], d["col"], val, y, 0.1, 0.0, 1e-4, 1e-4, threads=4)
    np.testing.assert_allclose(trainer.rmse_history, hist, rtol=1e-5)
    assert np.linalg.norm(fm.v - v) <= 1e-4 * np.linalg.norm(v)


@pytest.mark.parametrize("flat", [0, 1])
def test_random_shapes_property(fmhip, flat):
    """Property test over random shapes (hypothesis-style, fixed seeds so the GPU box runs the same
    cases): rows/features/k/batch size/row-length law vary; GPU gradient and one SGD epoch vs the oracle.
    flat=1 repeats it on the flat-address forward and the plain backward walk (fmhip_tune key 8) — the
    kernels that tables of 4 GiB and more select."""
    from sparkfm_amd import _ffi
    L = _ffi.load()
    L.fmhip_tune(_ffi.TUNE_FLAT_ADDRESS, flat)
    try:
        _random_shapes(fmhip, L)
    finally:
        L.fmhip_tune(_ffi.TUNE_FLAT_ADDRESS, 0)


@pytest.mark.parametrize("flat", [0, 1])
def test_random_shapes_property_of_wide_models(fmhip, flat):
    """The same property over models of 65..256 factors (Kp = 128 and 256, packed rows and full ones), seeds of their own."""
    from sparkfm_amd import _ffi
    L = _ffi.load()
    L.fmhip_tune(_ffi.TUNE_FLAT_ADDRESS, flat)
    try:
        _random_shapes(fmhip, L, seed=20261015, cases=16, ks=(65, 100, 128, 129, 200, 256))
    finally:
        L.fmhip_tune(_ffi.TUNE_FLAT_ADDRESS, 0)


def _random_shapes(fmhip, L, seed=20261003, cases=40, skip_diverged=False, ks=(1, 2, 5, 8, 13, 16, 32, 40, 64)):
    rng = np.random.default_rng(seed)
    for case in range(cases):
        k = int(rng.choice(list(ks)))
        n_rows = int(rng.integers(1, 1200))
        n1 = int(rng.integers(2, 400)) if case < 24 else int(rng.integers(400, 6000))   # wide models: rows-only update
        hi = int(rng.integers(1, min(n1, 70) + 1))
        lo = int(rng.integers(0, hi + 1))
        batch_rows = int(rng.choice([0, 1, 7, 64, 300, 5000]))
        a = random_problem(1000 + case + (seed - 20261003) * 1000, n_rows, n1, k, lo, hi, empty_rows=tuple(rng.integers(0, n_rows, 2).tolist()))
        if case % 3 == 0 and len(a["col"]):                          # a few dominating features
            hot = rng.integers(0, n1, 2)
            for r in range(n_rows):
                s = slice(a["row_ptr"][r], a["row_ptr"][r + 1])
                if s.stop - s.start >= 2 and not np.isin(hot, a["col"][s]).any():
                    a["col"][s.start] = hot[0]
        regs = (0.01, 0.01, 0.01) if case % 4 else (0.0, 0.0, 0.0)   # no decay: the fused step may update touched rows only
        try:
            L.fmhip_tune(_ffi.TUNE_HOT_BLOCK, 0 if case % 5 == 4 else 1)               # dense hot block off in a fifth of the cases
            ds, fm = make(fmhip, a, batch_rows=batch_rows)
        finally:
            L.fmhip_tune(_ffi.TUNE_HOT_BLOCK, 1)
        info = ds.info()
        nb = info["n_batches"]
        b = int(rng.integers(0, nb))
        bi = ds.batch_info(b)
        r0, r1 = bi["row0"], bi["row0"] + bi["rows"]
        assert bi["nnz"] == a["row_ptr"][r1] - a["row_ptr"][r0], case
        gv, gw, g0, st = fm.batchGradient(ds, b)
        ogv, ogw, og0, osse, oe = oracle.batch_grad(a["w0"], a["w"], a["v"], r0, r1, a["row_ptr"], a["col"], a["val"], a["y"])
        p0, p1 = int(a["row_ptr"][r0]), int(a["row_ptr"][r1])
        absw, terms = np.zeros(n1), np.zeros(n1)
        cb, xb = a["col"][p0:p1], a["val"][p0:p1]
        rb = np.repeat(np.arange(r1 - r0), np.diff(a["row_ptr"][r0:r1 + 1]))
        ex = np.abs(np.asarray(oe)[rb] * xb)
        np.add.at(absw, cb, ex)
        qrow = np.zeros((r1 - r0, k))
        np.add.at(qrow, rb, (a["v"][:, cb] * xb).T)                  # q_r = sum v x, per factor
        # sum |x| (|q| + |x v|) * (|e| + the forward's own fp32 error in e: ~ an ulp of the row's terms): a feature whose only
        # row has a small residual inherits that residual's RELATIVE error
        e_err = np.abs(np.asarray(oe))[rb] + 0.15 * term_scale(a)[r0:r1][rb]
        np.add.at(terms, cb, e_err * np.abs(xb) * (np.abs(qrow).max(axis=1)[rb] + np.abs(xb) * np.abs(a["v"][:, cb]).max(axis=0)))
        w_terms = np.zeros(n1)
        np.add.at(w_terms, cb, e_err * np.abs(xb))                   # the same for G_w = sum e x
        try:
            check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max(), cancelled=float(absw.max()) if len(absw) else 0.0, terms=terms, w_terms=w_terms)
        except AssertionError as e:
            raise AssertionError("case %d seed %d: k=%d rows=%d n1=%d nnz/row %d..%d batch_rows=%d batch %d: %s" % (case, seed, k, n_rows, n1, lo, hi, batch_rows, b, e))
        # sse = sum e^2 with |de| <= TOL_Y * O(1) per row  =>  |d sse| <= 2 * TOL_Y * sqrt(rows * sse)  (a single row
        # whose prediction nearly equals its label has a tiny e and a large RELATIVE error in e^2)
        assert st["rows"] == r1 - r0, case
        assert st["sse"] == pytest.approx(osse, rel=1e-5, abs=4 * TOL_Y * math.sqrt(max(osse, 0.0) * (r1 - r0)) + 1e-9), case
        feat, ptr, trows, tvals = ds.transposeInput(b)               # every stored entry, hot block or not
        assert len(trows) == bi["nnz"] and ptr[-1] == bi["nnz"], case
        np.testing.assert_array_equal(feat, np.unique(a["col"][a["row_ptr"][r0]:a["row_ptr"][r1]]).astype(np.int32))
        br = info["batch_rows"]
        eta = 0.02 if br >= 64 else 0.001                            # per-row SGD on long rows diverges at 0.02
        sgd = fmhip.HipSGD(eta=eta, reg0=regs[0], regw=regs[1], regv=regs[2])
        sgd.learn(fm, ds)
        w0, w, v, sse = oracle.sgd_epoch(a["w0"], a["w"], a["v"], br, a["row_ptr"], a["col"], a["val"], a["y"],
                                         eta, *regs)
        if skip_diverged and not (np.isfinite(v).all() and np.abs(v).max() < 1e3):   # (the soak's seeds: a case whose SGD diverges says nothing)
            ds.unpersist()
            fm.close()
            continue
        assert np.isfinite(v).all(), (case, "oracle diverged: pick a smaller eta for this case")
        slack = 0.0
        if skip_diverged:
            # the soak's seeds include nearly divergent trainings that amplify ANY rounding a thousandfold (k = 100, 60 entries
            # per row, eta 0.02: an initial perturbation of 1e-8 is 3e-5 after 15 steps): measure the case's own sensitivity —
            # the same fp64 epoch on the inputs rounded to fp32, which is what the GPU is given — and allow a multiple of it
            r32 = lambda x: np.asarray(x, np.float64).astype(np.float32).astype(np.float64)
            _, _, v32, _ = oracle.sgd_epoch(float(r32(a["w0"])), r32(a["w"]), r32(a["v"]), br, a["row_ptr"], a["col"], r32(a["val"]), r32(a["y"]), eta, *regs)
            slack = 30.0 * float(np.linalg.norm(v32 - v)) if np.isfinite(v32).all() else float("inf")
        assert np.linalg.norm(fm.v - v) <= 1e-5 * max(np.linalg.norm(v), 1e-9) + slack, (case, k, n_rows, n1, batch_rows)
        assert np.linalg.norm(fm.w - w) <= 1e-5 * max(np.linalg.norm(w), 1e-9) + slack, case
        assert fm.w0 == pytest.approx(w0, rel=1e-5, abs=1e-6 + slack), case      # (hundreds of per-row fp32 steps leave w0 a few ulps of its LARGEST past value off)
        ds.unpersist()
        fm.close()


@pytest.mark.parametrize("overlap,k", [(True, 32), (False, 32), (True, 16)])
def test_two_ranks_on_one_gpu(fmhip, tmp_path, overlap, k):
    """The real data-parallel path with TWO processes (both on cuda:0, collective over gloo): HipEngine,
    feature-chunked backward + async all-reduces (overlap) or one all-reduce per step, uneven shards
    (rank 1 runs out of batches first and contributes zero gradients).  Replicas must end bit-identical
    and match the oracle run over the equivalent global batches."""
    import socket
    import subprocess
    import sys
    from sparkfm_amd import synth
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = str(s.getsockname()[1])
    s.close()
    out = str(tmp_path / "dp")
    here = os.path.dirname(os.path.abspath(__file__))
    procs = [subprocess.Popen([sys.executable, os.path.join(here, "dist_gpu_worker.py"), str(r), "2", port, out,
                               "1" if overlap else "0", str(k)]) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=300) == 0
    r0, r1 = np.load(out + ".0.npz"), np.load(out + ".1.npz")
    np.testing.assert_array_equal(r0["v"], r1["v"])
    np.testing.assert_array_equal(r0["w"], r1["w"])
    assert float(r0["w0"]) == float(r1["w0"])
    if overlap:
        assert list(r0["cuts"]) == list(r1["cuts"]) and r0["cuts"][0] == 0 and r0["cuts"][-1] == 800 and len(r0["cuts"]) == 3
    # oracle: global batch j = rank0's batch j  U  rank1's batch j (rank 0 has 3 batches, rank 1 only 2: in the
    # last step of every epoch it contributes a zero gradient — HipEngine.compute_empty)
    shards = [synth.make_zipf(77, 3000, 800, 4, 24, zipf_s=1.05, row_begin=0),
              synth.make_zipf(77, 1700, 800, 4, 24, zipf_s=1.05, row_begin=3000)]
    w0, w, v = synth.init_params(5, 800, k, stdev=0.05)
    w = np.random.default_rng(9).normal(0, 0.05, 800)
    for _ in range(2):
        for j in range(3):
            rp, cols, vals, ys = [0], [], [], []
            for d in shards:
                n = len(d["y"])
                b0, b1 = j * 1000, min(n, (j + 1) * 1000)
                for r in range(b0, max(b0, b1)):
                    a, b = d["row_ptr"][r], d["row_ptr"][r + 1]
                    cols.append(d["col"][a:b])
                    vals.append(d["val"][a:b].astype(np.float64))
                    rp.append(rp[-1] + (b - a))
                    ys.append(float(d["y"][r]))
            w0, w, v, _ = oracle.sgd_step(w0, w, v, 0, len(ys), np.array(rp, np.int64), np.concatenate(cols),
                                          np.concatenate(vals), np.array(ys), 0.05, 0.0, 1e-3, 1e-3)
    assert np.linalg.norm(r0["v"] - v) <= 1e-5 * np.linalg.norm(v)
    assert np.linalg.norm(r0["w"] - w) <= 1e-5 * np.linalg.norm(w)
    assert float(r0["w0"]) == pytest.approx(w0, rel=1e-5, abs=1e-7)


@pytest.mark.parametrize("k,flat", [(32, 0), (32, 1), (64, 0), (128, 0), (256, 0), (128, 1), (256, 1)])
def test_the_residual_rides_in_the_p_row_exactly(fmhip, k, flat):
    """k == Kp leaves a P row no spare slot, so the forward writes the 32 bits of e into the low mantissa bits of the row's first
    floats and the backward reads them back from the row it gathers anyway (fm_device.h: no e gather).  e must arrive EXACTLY:
    every row gets a feature of its own with x = 1, whose G_w = sum e x is then that row's residual bit for bit — compared with
    the residuals the scoring pass returns, over values of every sign and magnitude (labels from 1e-30 to 1e+30, zero, negative)."""
    from sparkfm_amd import _ffi
    L = _ffi.load()
    rng = np.random.default_rng(k)
    n_rows, n_shared = 3000, 40
    n1 = n_shared + n_rows
    rows_c, rows_v = [], []
    for r in range(n_rows):
        sh = rng.choice(n_shared, size=int(rng.integers(1, 6)), replace=False)
        rows_c.append(np.concatenate([sh, [n_shared + r]]))
        rows_v.append(np.concatenate([rng.uniform(0.1, 1.0, len(sh)), [1.0]]))
    row_ptr = np.concatenate([[0], np.cumsum([len(c) for c in rows_c])]).astype(np.int64)
    col = np.concatenate(rows_c).astype(np.int32)
    val = np.concatenate(rows_v)
    y = rng.normal(0, 1, n_rows) * 10.0 ** rng.integers(-30, 31, n_rows)
    y[:8] = [0.0, -0.0, 1e-38, -1e-38, 3e38, -3e38, 1.0, -1.0]
    a = dict(k=k, n1=n1, w0=0.01, w=rng.normal(0, 0.05, n1), v=rng.normal(0, 0.05, (k, n1)), row_ptr=row_ptr, col=col, val=val, y=y)
    L.fmhip_tune(_ffi.TUNE_FLAT_ADDRESS, flat)
    try:
        ds, fm = make(fmhip, a, batch_rows=0)
        e = fm.residual(ds).astype(np.float32)
        _, gw, _, _ = fm.batchGradient(ds, 0)
    finally:
        L.fmhip_tune(_ffi.TUNE_FLAT_ADDRESS, 0)
    got = gw[n_shared:].astype(np.float32)
    assert np.array_equal(got.view(np.uint32), e.view(np.uint32)), int((got.view(np.uint32) != e.view(np.uint32)).sum())
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("k,hot", [(32, 1), (32, 0), (16, 1), (64, 1), (5, 0)])
def test_two_pass_forward_equals_the_forward(fmhip, k, hot):
    """fmhip_dataset_partition_rows + fmhip_step_forward_pass (pass 0: the features below a cut, pass 1: the others and the row's
    finish) against fmhip_step_forward: the same residual statistics and the same gradient up to the order of the forward's fp32
    sums, for a cut in the middle, a cut at 0 (everything in pass 1), a cut above every id (everything in pass 0), padded and
    unpadded and packed rows, with and without the dense hot block — and against the fp64 oracle."""
    import ctypes as C
    import torch
    from sparkfm_amd import _ffi, synth
    from sparkfm_amd.distributed import HipEngine
    L = _ffi.load()
    _ffi.check(L.fmhip_tune(_ffi.TUNE_HOT_BLOCK, hot))
    try:
        n1 = 900
        d = synth.make_zipf(515 + k, 6000, n1, 3, 28, zipf_s=1.05)
        rng = np.random.default_rng(k)
        a = dict(n1=n1, k=k, row_ptr=d["row_ptr"], col=d["col"], val=d["val"].astype(np.float64), y=d["y"].astype(np.float64),
                 w0=0.1, w=rng.normal(0, 0.05, n1), v=rng.normal(0, 0.05, (k, n1)))
        ds, fm = make(fmhip, a, batch_rows=3000, stream=torch_stream())
        assert (ds.layout()["hot_pages"] > 0) == bool(hot)
        eng = HipEngine(fm, ds)
        ogv, ogw, og0, osse, _ = oracle.batch_grad(a["w0"], a["w"], a["v"], 3000, 6000, a["row_ptr"], a["col"], a["val"], a["y"], threads=8)
        head = 32

        def grad_of(run):
            eng.grad.zero_()
            torch.cuda.synchronize()
            _ffi.check(L.fmhip_grad_bind(fm.handle, C.c_void_p(eng.grad.data_ptr())))
            run()
            torch.cuda.synchronize()
            return eng.grad.clone().cpu().numpy().astype(np.float64)

        def two_pass():
            _ffi.check(L.fmhip_step_forward_pass(fm.handle, ds.handle, 1, 0))
            _ffi.check(L.fmhip_step_forward_pass(fm.handle, ds.handle, 1, 1))
            eng.backward(1, 0, n1, finish=True)

        want = grad_of(lambda: eng.compute(1))
        assert L.fmhip_step_forward_pass(fm.handle, ds.handle, 1, 0) != 0 and b"not partitioned" in L.fmhip_last_error()
        for cut in (120, 0, n1, 7):
            _ffi.check(L.fmhip_dataset_partition_rows(ds.handle, cut))
            plain = grad_of(lambda: eng.compute(1))                  # the plain forward over the re-ordered rows: the same sums, another order
            got = grad_of(two_pass)
            scale = np.abs(want[head:]).max()
            for name, g in (("plain", plain), ("two-pass", got)):
                assert np.abs(g[head:] - want[head:]).max() <= 2e-5 * scale, (name, cut, float(np.abs(g[head:] - want[head:]).max() / scale))
                np.testing.assert_allclose(g[:2], want[:2], rtol=2e-5, atol=1e-4, err_msg="%s %d" % (name, cut))   # sum e, sum e^2
                assert g[2] == 3000.0
            assert abs(got[1] - osse) <= 1e-5 * osse
        gv, gw, _, _ = fm.batchGradient(ds, 1)
        check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
        eng.close()
        ds.unpersist()
        fm.close()
    finally:
        _ffi.check(L.fmhip_tune(_ffi.TUNE_HOT_BLOCK, 1))


def test_partitioned_rows_keep_the_als_learner_right(fmhip):
    """fmhip_dataset_partition_rows on a single-batch dataset: the fp64 copy of the values the ALS learner reads beside the column
    ids moves with them — two ALS epochs on partitioned rows equal the oracle's (and the unpartitioned run) to fp64 reassociation."""
    from sparkfm_amd import _ffi
    L = _ffi.load()
    a = random_problem(516, 1200, 100, 5, 0, 12, empty_rows=(3,))
    rng = np.random.default_rng(4)
    a["y"] = oracle.predict(0.3, rng.normal(0, 0.3, 100), rng.normal(0, 0.3, (3, 100)), a["row_ptr"], a["col"], a["val"]) + rng.normal(0, 0.05, 1200)
    out = []
    for cut in (None, 37):
        ds, fm = make(fmhip, a)
        if cut is not None:
            _ffi.check(L.fmhip_dataset_partition_rows(ds.handle, cut))
        fm.reg0, fm.regw, fm.regv = 0.0, 0.1, 10.0
        for _ in range(2):
            fmhip.HipALS.run().learn(fm, ds)
        out.append((fm.w0, fm.w.copy(), fm.v.copy()))
        ds.unpersist()
        fm.close()
    w0, w, v = a["w0"], a["w"], a["v"]
    for _ in range(2):
        w0, w, v = oracle.als_epoch(w0, w, v, 0.0, 0.1, 10.0, a["row_ptr"], a["col"], a["val"], a["y"])
    for got in out:
        np.testing.assert_allclose(got[2], v, rtol=1e-8, atol=1e-11)
        np.testing.assert_allclose(got[1], w, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(out[1][2], out[0][2], rtol=1e-10, atol=1e-13)


@pytest.mark.parametrize("k", [8, 65])
def test_scoring_calls_share_one_pass(fmhip, k):
    """What the scoring calls have in common because they run ONE pass (fmhip_score.hip): fmhip_auc's statistics are fmhip_rmse's,
    bit for bit; fmhip_predict from four threads at once is the serial call; fmhip_residual is predict - y in fp32.  1,000 rows x
    300 features in batches of 384, 384 and 232 rows, packed rows with 8-lane (k = 8) and 16-lane slots (k = 65); the model is
    1,001 features wide, so that the SGD epoch's weight decay stays in the tables' scales (sv, sw != 1) when the calls read them."""
    import ctypes as C
    import threading
    from sparkfm_amd import _ffi, synth
    d = synth.make_zipf(7, 1000, 300, 4, 12, zipf_s=1.05)
    ds = fmhip.DataSet.from_arrays(d, batch_rows=384).cache()
    assert [ds.batch_info(b)["rows"] for b in range(ds.n_batches)] == [384, 384, 232]
    fm = fmhip.FMModel(1000, k)
    rng = np.random.Generator(np.random.PCG64(11 + k))
    fm.w0, fm.w, fm.v = 0.1, rng.normal(0.0, 0.05, 1001), rng.normal(0.0, 0.05, (k, 1001))
    fmhip.HipSGD(eta=0.05, regw=1e-3, regv=1e-3).learn(fm, ds)
    L, r, st_rmse = _ffi.load(), C.c_double(), _ffi.Stats()
    _ffi.check(L.fmhip_rmse(fm.handle, ds.handle, C.byref(r), C.byref(st_rmse)))
    st_auc = fm.aucDetails(ds, stats=True)["stats"]
    assert st_rmse.rows == 1000 and st_rmse.nonfinite == 0 and st_rmse.nnz == len(d["col"])
    for name, _ in _ffi.Stats._fields_:
        assert np.array(getattr(st_rmse, name)).tobytes() == np.array(st_auc[name]).tobytes(), name
    serial = fm.predict(ds)
    got = [None] * 4

    def score(i):
        got[i] = fm.predict(ds)
    threads = [threading.Thread(target=score, args=(i,)) for i in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for g in got:
        assert g is not None and g.tobytes() == serial.tobytes()
    e32 = serial.astype(np.float32) - ds.y.astype(np.float32)
    assert e32.dtype == np.float32 and fm.residual(ds).tobytes() == e32.astype(np.float64).tobytes()
    ds.unpersist()
    fm.close()
