"""The second trip of the finishes' grid-strided loops (fm_finish.h: SlotLoop, slot_blocks).  A finish launches at most 8192
workgroups of 256 / LPN slots, and a slot whose first item lies below the count takes the item one grid further on too: one batch
of 8192 * slots + a few items sends the first slots round twice, which no other test's batch is long enough for.

The relational finish's case is a step against relational_ref.py and says so itself.  Every other case is one batch of rows
with 2 entries each over 64 features, its gradient and statistics against the fp64 twins
(weight_ref.py / train_ref.py: the oracle at the pseudo-targets y' = yhat - e) at the tolerances of the gradient tests next door:
check_grad of test_gpu_parity.py as test_gpu_pairing.check_batches uses it, sse to rel 1e-5, sum e as test_gpu_weights.py's
test_one_step_vs_twin (pairs: exactly 0).  The rows of the second trip are made to matter — they walk the features two by two, so
every feature has some, with the largest weight by far (pairs: with one label order, so their residuals have one sign) — and the
twin alone shows, before anything runs on the device, that leaving them out moves every entry of gw by more than ten times its
tolerance."""
import numpy as np
import pytest

import oracle
import relational_ref as rref
import train_ref as ref
import weight_ref as wref
from test_gpu_parity import TOL_G, check_grad
from test_gpu_relational import check_stats
from test_gpu_weights import check_step

pytestmark = pytest.mark.gpu

N1 = 64
CAP = 8192          # slot_blocks' cap on the grid


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def two_entry_rows(seed, n_rows, n_tail, k):
    """n_rows rows of 2 distinct features of [0, 64) each, values in [0.25, 1]: random ones, but the last n_tail rows take the
    features two by two (row t of them: 2t and 2t + 1 mod 64); parameters N(0, 0.1)."""
    rng = np.random.default_rng(seed)
    first = rng.integers(0, N1, n_rows)
    col = np.stack([first, (first + rng.integers(1, N1, n_rows)) % N1], axis=1).astype(np.int32)
    col[n_rows - n_tail:] = (2 * np.arange(n_tail)[:, None] + np.arange(2)[None, :]) % N1
    col = col.reshape(-1)
    val = rng.uniform(0.25, 1.0, 2 * n_rows)
    return dict(k=k, n1=N1, row_ptr=np.arange(n_rows + 1, dtype=np.int64) * 2, col=col, val=val, w0=float(rng.normal(0, 0.1)),
                w=rng.normal(0, 0.1, N1), v=rng.normal(0, 0.1, (k, N1)))


def check(fmhip, a, c, loss, pairs, first_trip_rows):
    from sparkfm_amd import _ffi
    n = len(a["y"])
    rule = wref.Rule(loss, pairs, None)
    ones = np.ones(n) if c is None else c
    yp, e, _ = wref.pseudo_targets(wref.State(a["w0"], a["w"], a["v"]), a["row_ptr"], a["col"], a["val"], a["y"], ones, rule)
    grad = lambda r1: oracle.batch_grad(a["w0"], a["w"], a["v"], 0, r1, a["row_ptr"], a["col"], a["val"], yp)      # noqa: E731
    ogv, ogw, og0, osse, oe = grad(n)
    np.testing.assert_allclose(oe, e, rtol=1e-12, atol=1e-12)        # the oracle's residual at y' IS the rule's
    # the twin alone: without the second trip's rows gw is another gradient, by far more than check_grad allows
    gw_tol = TOL_G * (np.abs(ogw) + max(np.abs(ogw).max(), 1e-6))
    moved = np.abs(ogw - grad(first_trip_rows)[1]) / gw_tol
    print("second trip: %d rows, move gw by %.3g .. %.3g tolerances" % (n - first_trip_rows, moved.min(), moved.max()))
    assert n > first_trip_rows and (moved > 10).all()

    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=0, weights=c).cache()
    fm = fmhip.FMModel(N1 - 1, a["k"])
    fm.w0, fm.w, fm.v = a["w0"], a["w"], a["v"]
    L = _ffi.load()
    _ffi.check(L.fmhip_model_set_loss(fm.handle, _ffi.loss_code(loss)))
    _ffi.check(L.fmhip_model_set_pairing(fm.handle, _ffi.pairing_code(pairs)))
    assert ds.n_batches == 1
    gv, gw, g0, st = fm.batchGradient(ds, 0)
    print("max |gv - twin| %.3g, max |gw - twin| / tolerance %.3g, sse rel %.3g, sum_e %.9g (twin %.9g)"
          % (np.abs(gv - ogv).max(), (np.abs(gw - ogw) / gw_tol).max(), abs(st["sse"] / osse - 1), st["sum_e"], e.sum()))
    check_grad(gv, gw, ogv, ogw, np.abs(a["v"]).max())
    assert st["rows"] == n and st["nonfinite"] == 0
    assert st["sse"] == pytest.approx(osse, rel=1e-5) and osse == pytest.approx((e * e).sum(), rel=1e-12)
    if pairs:
        assert g0 == 0.0 and st["sum_e"] == 0.0
    else:
        assert st["sum_e"] == pytest.approx(e.sum(), rel=1e-5, abs=1e-4) and g0 == pytest.approx(og0, rel=1e-5, abs=1e-4)
    ds.unpersist()
    fm.close()


def weighted_rows(seed, n_head, n_tail, k, loss):
    """n_head rows with weights from {0, 0.25, 1, 3.5}, then n_tail rows of weight 64 whose labels give their residuals one sign
    (logistic: all positive, e = sigma - 1 < 0; squared: y = -3, e = yhat + 3 > 0)."""
    n = n_head + n_tail
    a = two_entry_rows(seed, n, n_tail, k)
    rng = np.random.default_rng(seed + 1)
    a["y"] = (rng.random(n) < 0.4).astype(np.float64) if loss == "logistic" else rng.normal(0.5, 1.0, n)
    a["y"][n_head:] = 1.0 if loss == "logistic" else -3.0
    return a, np.concatenate([wref.draw_weights(seed + 2, n_head), np.full(n_tail, 64.0)])


def test_weight_finish_second_trip_lpn8(fmhip):
    """k = 8 (Kp = 32, 32 slots per workgroup, e in the packed slot): 8192 * 32 + 64 weighted logistic rows."""
    a, c = weighted_rows(71, CAP * 32, 64, 8, "logistic")
    check(fmhip, a, c, "logistic", False, CAP * 32)


def test_pair_finish_second_trip(fmhip):
    """k = 8: 8192 * 32 + 64 logistic pairs.  The last 64 pairs prefer their first row, every one (g = sigma(d) - 1 < 0), and a
    feature lies always in the first or always in the second row of them: what they add to a feature's gw has one sign."""
    n_head, n_tail = CAP * 32, 64
    a = two_entry_rows(72, 2 * (n_head + n_tail), 2 * n_tail, 8)
    a["y"] = (np.random.default_rng(73).random(2 * (n_head + n_tail)) < 0.4).astype(np.float64)
    a["y"][2 * n_head:] = np.tile([1.0, 0.0], n_tail)
    check(fmhip, a, None, "logistic", True, 2 * n_head)


def test_weight_finish_second_trip_lpn16(fmhip):
    """k = 100 (Kp = 128, 16 slots per workgroup): 8192 * 16 + 32 weighted squared-loss rows."""
    a, c = weighted_rows(74, CAP * 16, 32, 100, "squared")
    check(fmhip, a, c, "squared", False, CAP * 16)


def test_rel_finish_second_trip(fmhip):
    """k = 8, squared loss: 8192 * 32 + 64 data rows over two 16-row blocks (features [0, 32) and [32, 64)), no plain part — one
    relational step against relational_ref.py in the form of test_gpu_relational.test_one_step_vs_twin (check_step, check_stats).
    Every block row is referenced by 16 k rows: the segmented sum takes its long lists' two passes.  The last 64 rows have the
    label -50 (e = yhat + 50 > 0) and walk the block rows one by one; the step size is 5, so that a step over 262 k rows moves the
    parameters by more than their fp32 spacing (check_step asserts that it moved)."""
    n_head, n_tail, k, eta = CAP * 32, 64, 8, 5.0
    n = n_head + n_tail
    rng = np.random.default_rng(75)
    blocks = [rref.random_block(rng, 16, 2, 5, 0, 32), rref.random_block(rng, 16, 2, 5, 32, 64)]
    maps = [np.concatenate([rng.integers(0, 16, n_head), np.arange(n_tail) % 16]) for _ in blocks]
    p = rref.make_problem(76, n, k, blocks, maps, None, N1)
    p["y"][n_head:] = -50.0
    s0 = ref.State(p["w0"], p["w"], p["v"], 0.0)
    e = rref.residuals(s0, p, 0, n, "squared")
    s1 = rref.step(s0.copy(), p, 0, n, eta, 0.0, 0.0, 0.0)
    # the twin alone: a step without the second trip's rows' residuals moves w elsewhere, by far more than check_step allows
    gw, gw_head = rref.gradient(s0, p, 0, n, "squared")[1], rref.gradient(s0, p, 0, n_head, "squared")[1]
    seen = gw != 0                                                          # (a block stores 2-5 features per row: not every id occurs)
    moved = np.abs(gw - gw_head)[seen] / (2 * TOL_G * np.abs(gw).max())
    print("second trip: %d rows, move gw by %.3g .. %.3g tolerances" % (n_tail, moved.min(), moved.max()))
    assert seen.sum() > N1 // 2 and (moved > 10).all()

    rd, fm = rref.build(fmhip, p)
    st = fmhip.HipSGD(eta=eta, loss="squared").step(fm, rd, 0)
    print("max |dw - twin| %.3g of max |dw| %.3g, sse rel %.3g, sum_e %.9g (twin %.9g)"
          % (np.abs((fm.w - s0.w) - (s1.w - s0.w)).max(), np.abs(s1.w - s0.w).max(), abs(st["sse"] / (e * e).sum() - 1), st["sum_e"], e.sum()))
    check_step(fm, s0, s1)
    check_stats(st, e)
    rd.unpersist()
    for part in rd._parts():
        part.unpersist()
    fm.close()
