"""Models of 65..256 factors — padded widths Kp = 128 and 256, the template instances with J = 2 and 4 float4s per lane — on every
kernel path against the fp64 oracle.

include/fmhip.h promises up to FMHIP_MAX_FACTORS = 256 factors.  A row of V (and of P) is Kp floats, a node's LPN lanes hold J
float4s each (Kp = 4 * LPN * J).  When k < Kp, slot k of a V row carries the feature's linear weight and slot k of a P row the
residual e; it sits in float4 j = (k >> 2) / LPN of lane (k >> 2) & (LPN - 1), component k & 3.  The set of k below puts that
slot at the first and last float4 of each wide geometry, at its first and last lane and component, and includes k == Kp (no
spare slot: e rides in the P row's low mantissa bits):

    k     Kp    (kj, kl, kc)          k     Kp    (kj, kl, kc)
    65    128   (1, 0, 1)             160   256   (2, 8, 0)
    127   128   (1, 15, 3)            200   256   (3, 2, 0)
    129   256   (2, 0, 1)             255   256   (3, 15, 3)
    131   256   (2, 0, 3)             128, 256    none

Tolerances as in test_gpu_parity.py."""
import numpy as np
import pytest

import oracle
from helpers import random_problem
from sparkfm_amd import _ffi  # noqa: F401  (the tuning keys' names)
from test_gpu_parity import TOL_Y, check_grad, make, term_scale
from test_gpu_world8 import case8, check_dense_or_sharded, padded_factors, run_case

pytestmark = pytest.mark.gpu

WIDE_K = [65, 127, 128, 129, 131, 160, 200, 255, 256]


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def slot_factors(k):
    """Factor 0, the last factor, the factors that share the packed slot's float4 (or the last float4) and one in the middle."""
    return sorted({0, k // 2, k - 1, max(k - 2, 0), 4 * ((k - 1) // 4)} | ({4 * (k // 4) - 1} if k >= 4 else set()))


def wide_problem(k, seed=0):
    """4 ragged batches of 300 rows; empty rows; unsorted indices; feature 0 present in every non-empty row."""
    a = random_problem(9100 + k + seed, 1000, 257, k, 0, 40, empty_rows=(0, 17, 999))
    for r in range(1000):
        s = slice(a["row_ptr"][r], a["row_ptr"][r + 1])
        if s.stop > s.start and not (a["col"][s] == 0).any():
            a["col"][s.start] = 0
    return a


@pytest.mark.parametrize("k", WIDE_K)
def test_forward_gradient_and_step_of_wide_models(fmhip, k):
    """Predictions (empty rows exactly w0), residual, RMSE, termQ beside the packed slot, every batch's G_V / G_w / g0 / sse, one
    SGD step, and the parameters read back through the API after a step that changes nothing (the packed slot's round trip)."""
    a = wide_problem(k)
    ds, fm = make(fmhip, a, batch_rows=300)
    assert ds.info()["n_batches"] == 4
    sc = term_scale(a)
    yh = fm.predict(ds)
    oyh = oracle.predict(a["w0"], a["w"], a["v"], a["row_ptr"], a["col"], a["val"])
    assert (np.abs(yh - oyh) <= TOL_Y * sc).all(), float((np.abs(yh - oyh) / sc).max())
    for r in (0, 17, 999):
        assert yh[r] == np.float32(a["w0"])
    e = fm.residual(ds)
    oe = oracle.residual(a["w0"], a["w"], a["v"], a["row_ptr"], a["col"], a["val"], a["y"])
    assert (np.abs(e - oe) <= TOL_Y * sc).all(), float((np.abs(e - oe) / sc).max())
    assert fm.computeRMSE(ds) == pytest.approx(oracle.rmse(a["w0"], a["w"], a["v"], a["row_ptr"], a["col"], a["val"], a["y"]), rel=1e-5)
    q = fm.termQ(ds)
    assert q.shape == (1000, k)
    cp, rows, cv = oracle.transpose(a["n1"], a["row_ptr"], a["col"], a["val"])
    for ff in slot_factors(k):
        np.testing.assert_allclose(q[:, ff], oracle.term_q(a["v"], ff, 1000, cp, rows, cv), rtol=1e-5, atol=1e-5, err_msg="factor %d" % ff)
    for b in range(4):
        r0, r1 = b * 300, min(1000, (b + 1) * 300)
        gv, gw, g0, st = fm.batchGradient(ds, b)
        ogv, ogw, og0, osse, _ = oracle.batch_grad(a["w0"], a["w"], a["v"], r0, r1, a["row_ptr"], a["col"], a["val"], a["y"])
        check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
        assert g0 == pytest.approx(og0, rel=1e-5, abs=1e-4)
        assert st["sse"] == pytest.approx(osse, rel=1e-5)
        assert st["rows"] == r1 - r0 and st["nonfinite"] == 0
    regs = (0.01, 1e-3, 2e-3)
    st = fmhip.HipSGD(eta=0.05, reg0=regs[0], regw=regs[1], regv=regs[2]).step(fm, ds, 2)
    o0, ow, ov, osse = oracle.sgd_step(a["w0"], a["w"], a["v"], 600, 900, a["row_ptr"], a["col"], a["val"], a["y"], 0.05, *regs)
    assert st["sse"] == pytest.approx(osse, rel=1e-5)
    assert np.abs(fm.v - ov).max() <= 1e-6 + 1e-5 * np.abs(ov).max() and np.linalg.norm(fm.v - ov) <= 1e-5 * np.linalg.norm(ov)
    assert np.abs(fm.w - ow).max() <= 1e-6 + 1e-5 * np.abs(ow).max()
    assert fm.w0 == pytest.approx(o0, rel=1e-5, abs=1e-7)
    # set -> device -> read back: fp32-exact values through a step of eta 0 (the device copy becomes the only current one)
    rng = np.random.default_rng(k)
    w32 = rng.normal(0, 0.1, a["n1"]).astype(np.float32)
    v32 = rng.normal(0, 0.1, (k, a["n1"])).astype(np.float32)
    fm.w0, fm.w, fm.v = 0.5, w32.astype(np.float64), v32.astype(np.float64)
    fmhip.HipSGD(eta=0.0).step(fm, ds, 1)
    np.testing.assert_array_equal(fm.w.astype(np.float32).view(np.uint32), w32.view(np.uint32))
    np.testing.assert_array_equal(fm.v.astype(np.float32).view(np.uint32), v32.view(np.uint32))
    ids = np.array([0, 6, 256, 5, 7, 100], np.int32)
    w_r, v_r = fm.rows(ids)
    np.testing.assert_array_equal(w_r.astype(np.float32).view(np.uint32), w32[ids].view(np.uint32))
    np.testing.assert_array_equal(v_r.astype(np.float32).view(np.uint32), v32[:, ids].view(np.uint32))
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("fwd,tile", [(60, 0), (60, 16), (20, 0), (20, 16), (0, 0)])
@pytest.mark.parametrize("flat", [0, 1])
def test_kernel_variants_of_wide_models(fmhip, request, fwd, tile, flat):
    """The forward kernels (tuning key 0: the w-tile kernel 60, the LDS V-tile 20 with tile rows 0 / 16, the plain 0), each on
    buffer views and on flat addresses (key 8), at a packed Kp = 256 row (k = 200) and a full one (k = 256): the oracle's
    predictions, gradient and epoch.  Backward key 1 (the pipelined walk) takes the plain walk at Kp > 64: keys 0 and 1 give the
    same bits."""
    from sparkfm_amd import _ffi
    L = _ffi.load()

    def reset():
        L.fmhip_tune(_ffi.TUNE_FORWARD_KERNEL, 60), L.fmhip_tune(_ffi.TUNE_BACKWARD_KERNEL, 1)
        L.fmhip_tune(_ffi.TUNE_TILE_ROWS, 0), L.fmhip_tune(_ffi.TUNE_FLAT_ADDRESS, 0)
    request.addfinalizer(reset)
    L.fmhip_tune(_ffi.TUNE_FORWARD_KERNEL, fwd), L.fmhip_tune(_ffi.TUNE_TILE_ROWS, tile), L.fmhip_tune(_ffi.TUNE_FLAT_ADDRESS, flat)
    for k in (200, 256):
        a = random_problem(300 + k, 700, 300, k, 0, 30, empty_rows=(1, 699))
        ds, fm = make(fmhip, a, batch_rows=256)
        sc = term_scale(a)
        yh = fm.predict(ds)
        oyh = oracle.predict(a["w0"], a["w"], a["v"], a["row_ptr"], a["col"], a["val"])
        assert (np.abs(yh - oyh) <= TOL_Y * sc).all(), k
        assert yh[1] == np.float32(a["w0"]) and yh[699] == np.float32(a["w0"])
        grads = []
        for bwd in (0, 1):
            L.fmhip_tune(_ffi.TUNE_BACKWARD_KERNEL, bwd)
            grads.append(fm.batchGradient(ds, 1))
        (gv, gw, g0, st), (gv1, gw1, g01, st1) = grads
        np.testing.assert_array_equal(gv, gv1)
        np.testing.assert_array_equal(gw, gw1)
        assert g0 == g01 and st["sse"] == st1["sse"]
        ogv, ogw, og0, osse, _ = oracle.batch_grad(a["w0"], a["w"], a["v"], 256, 512, a["row_ptr"], a["col"], a["val"], a["y"])
        check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
        assert st["sse"] == pytest.approx(osse, rel=1e-5)
        sgd = fmhip.HipSGD(eta=0.03, regv=1e-3)
        sgd.learn(fm, ds)
        w0, w, v, sse = oracle.sgd_epoch(a["w0"], a["w"], a["v"], 256, a["row_ptr"], a["col"], a["val"], a["y"], 0.03, 0.0, 0.0, 1e-3)
        assert np.linalg.norm(fm.v - v) <= 1e-5 * np.linalg.norm(v), k
        assert np.linalg.norm(fm.w - w) <= 1e-5 * np.linalg.norm(w), k
        assert sgd.last_stats["sse"] == pytest.approx(sse, rel=1e-5)
        ds.unpersist()
        fm.close()


@pytest.mark.parametrize("k", [200, 256])
@pytest.mark.parametrize("order", [0, 1])
def test_row_order_of_wide_models_is_only_an_order(fmhip, request, k, order):
    """Tuning key 7: the rows of wide models walked longest-first, or in stored order; either way every row is visited once."""
    from sparkfm_amd import _ffi
    L = _ffi.load()
    request.addfinalizer(lambda: L.fmhip_tune(_ffi.TUNE_ROW_ORDER, 1))
    L.fmhip_tune(_ffi.TUNE_ROW_ORDER, order)
    a = random_problem(777 + k, 1500, 300, k, 0, 60, empty_rows=(3, 1499))
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


@pytest.mark.parametrize("exchange", ["dense", "sharded"])
def test_eight_ranks_dense_and_sharded_at_a_wide_model(tmp_path, exchange):
    """The library's data-parallel step with eight thread ranks at k = 200 (Kp = 256: k_apply_shard<256> in the sharded mode)."""
    cfg = case8(exchange=exchange, fractions=[0.3], k=200)
    check_dense_or_sharded(run_case(cfg, tmp_path), cfg)


def test_eight_ranks_touched_rows_at_a_wide_model(tmp_path):
    s = run_case(case8(exchange="touched", k=200, n1=2003), tmp_path)
    assert s["world"] == 8 and s["steps"] == 4 and s["rows"] == 200
    assert s["rel_err_v"] <= 1e-5 and s["rel_err_w"] <= 1e-5
    assert s["info"]["mode"] == "touched"


@pytest.mark.parametrize("k", [100, 256])
def test_pipelined_exchange_of_a_wide_model_is_the_dense_step(tmp_path, k):
    """The pipelined exchange needs the two-pass forward, which serves Kp <= 64: wider models take the dense step — the very same
    collectives as the dense mode, replicas bit-identical (the worker checks), the oracle matched."""
    got = {}
    for exchange in ("pipelined", "dense"):
        got[exchange] = run_case(case8(exchange=exchange, fractions=[0.05, 0.3], k=k), tmp_path)
        assert got[exchange]["rel_err_v"] <= 1e-5 and got[exchange]["rel_err_w"] <= 1e-5
    assert got["pipelined"]["calls"] == got["dense"]["calls"] and got["pipelined"]["cuts"] == got["dense"]["cuts"]
    assert got["pipelined"]["rel_err_v"] == got["dense"]["rel_err_v"] and got["pipelined"]["rel_err_w"] == got["dense"]["rel_err_w"]


@pytest.mark.parametrize("k", [100, 200])
def test_the_two_pass_forward_refuses_wide_models(fmhip, k):
    """fmhip_step_forward_pass on a Kp = 128 / 256 model: FMHIP_ERR_UNSUPPORTED with the limit in the message, nothing launched —
    the model trains like the oracle afterwards."""
    from sparkfm_amd import _ffi
    L = _ffi.load()
    a = random_problem(60 + k, 900, 200, k, 1, 20)
    ds, fm = make(fmhip, a, batch_rows=300)
    _ffi.check(L.fmhip_dataset_partition_rows(ds.handle, 100))
    for pass_ in (0, 1):
        assert L.fmhip_step_forward_pass(fm.handle, ds.handle, 1, pass_) == -5
        msg = L.fmhip_last_error()
        assert b"up to 64 padded factors" in msg and (b"this one: %d" % padded_factors(k)) in msg, msg
    sgd = fmhip.HipSGD(eta=0.05, regw=1e-3, regv=1e-3)
    sgd.learn(fm, ds)
    w0, w, v, sse = oracle.sgd_epoch(a["w0"], a["w"], a["v"], 300, a["row_ptr"], a["col"], a["val"], a["y"], 0.05, 0.0, 1e-3, 1e-3)
    assert sgd.last_stats["sse"] == pytest.approx(sse, rel=1e-5)
    assert np.linalg.norm(fm.v - v) <= 1e-5 * np.linalg.norm(v) and np.linalg.norm(fm.w - w) <= 1e-5 * np.linalg.norm(w)
    ds.unpersist()
    fm.close()


def test_als_epoch_of_a_wide_model(fmhip):
    """One ALS epoch (fp64 on the GPU) at k = 200 against the oracle's."""
    a = random_problem(5200, 600, 80, 200, 0, 12, empty_rows=(7,))
    rng = np.random.default_rng(12)
    a["y"] = oracle.predict(0.3, rng.normal(0, 0.3, 80), rng.normal(0, 0.3, (3, 80)), a["row_ptr"], a["col"], a["val"]) + rng.normal(0, 0.05, 600)
    ds, fm = make(fmhip, a)
    fm.reg0, fm.regw, fm.regv = 0.0, 0.1, 10.0
    fmhip.HipALS.run().learn(fm, ds)
    w0, w, v = oracle.als_epoch(a["w0"], a["w"], a["v"], 0.0, 0.1, 10.0, a["row_ptr"], a["col"], a["val"], a["y"])
    np.testing.assert_allclose(fm.v, v, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(fm.w, w, rtol=1e-8, atol=1e-11)
    assert fm.w0 == pytest.approx(w0, rel=1e-9)
    ds.unpersist()
    fm.close()
