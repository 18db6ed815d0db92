"""The pairing switch's host surface (no GPU): argument checks of fmhip_model_set_pairing / fmhip_pair_logloss, the learners'
`pairs=`, the header's enum against the binding's constants, DataSet.from_pairs, and the reference rule of train_ref.py
against finite differences of the pair loss."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import train_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_model_is_refused():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    assert L.fmhip_model_set_pairing(None, _ffi.PAIRING_ADJACENT) == -1
    assert b"NULL" in L.fmhip_last_error()
    assert L.fmhip_model_set_pairing(None, _ffi.PAIRING_NONE) == -1
    r, c = C.c_double(), C.c_double()
    assert L.fmhip_pair_logloss(None, None, C.byref(r), C.byref(c), None) == -1
    assert b"NULL" in L.fmhip_last_error()
    assert L.fmhip_pair_logloss(None, None, None, None, None) == -1


def test_unknown_pairing_value_is_refused():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    # the value is checked before the handle (a model needs a device): the message names it
    for bad in (7, -1, 2):
        assert L.fmhip_model_set_pairing(None, bad) == -1
        assert ("pairing %d" % bad).encode() in L.fmhip_last_error()
    # the loss's door is its own: a pairing is no loss
    assert L.fmhip_model_set_loss(None, 2) == -1
    assert b"loss 2" in L.fmhip_last_error()
    for bad in ("adjacent", 1, 0, None):
        with pytest.raises(ValueError, match="pairs"):
            _ffi.pairing_code(bad)
    assert _ffi.pairing_code(False) == _ffi.PAIRING_NONE and _ffi.pairing_code(True) == _ffi.PAIRING_ADJACENT


def test_learners_refuse_a_bad_keyword():
    from sparkfm_amd import HipSGD
    from sparkfm_amd.distributed import DataParallelSGD, HipDataParallelSGD
    with pytest.raises(ValueError):
        HipSGD(pairs="adjacent")
    with pytest.raises(ValueError):
        HipSGD.run(loss="logistic", pairs=1)
    with pytest.raises(ValueError):
        DataParallelSGD(pairs="yes")
    with pytest.raises(ValueError):
        HipDataParallelSGD(None, pairs=2)      # refused before the communicator is touched
    assert HipSGD().pairs is False and DataParallelSGD().pairs is False
    assert HipSGD.run(loss="logistic", pairs=True).pairs is True and DataParallelSGD(pairs=True).pairs is True


def test_data_parallel_engine_without_the_call_refuses_pairs():
    """DataParallelSGD sets the pairing through its engine before every step; an engine that cannot raises ValueError (as it
    does for a non-squared loss)."""
    from sparkfm_amd.distributed import DataParallelSGD

    class Engine:                      # no set_loss, no set_pairing, no set_optimizer
        n_batches = 1
        grad = None

        def compute(self, j):
            raise AssertionError("must not be reached")

    with pytest.raises(ValueError, match="single rows"):
        DataParallelSGD(pairs=True).step(Engine(), 0)


def test_header_enum_matches_the_binding():
    from sparkfm_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_pairing.h")).read()
    m = re.search(r"enum fmhip_pairing \{([^}]*)\}", hdr)
    assert m
    vals = dict((k, int(v)) for k, v in re.findall(r"FMHIP_PAIRING_([A-Z]+) = (\d+)", m.group(1)))
    assert vals == {"NONE": _ffi.PAIRING_NONE, "ADJACENT": _ffi.PAIRING_ADJACENT}
    declared = set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_PAIRING) == {"fmhip_model_set_pairing", "fmhip_pair_logloss"}
    assert not set(_ffi.SYMBOLS_PAIRING) & set(_ffi.SYMBOLS + _ffi.SYMBOLS_EXPERIMENTAL + _ffi.SYMBOLS_TOPK)
    assert re.search(r"int fmhip_model_set_pairing\(fmhip_model_t m, int pairing\);", hdr)
    assert re.search(r"int fmhip_pair_logloss\(fmhip_model_t m, fmhip_dataset_t d, double \*logloss, double \*concordance", hdr)
    L = _ffi.load()
    assert hasattr(L, "fmhip_model_set_pairing") and hasattr(L, "fmhip_pair_logloss")


def test_from_pairs_interleaves():
    from sparkfm_amd import DataSet
    pref = [([1, 5], [1.0, 0.5]), ([2], [2.0]), ([], [])]
    oth = [([3], [0.25]), ([4, 6, 7], [1.0, 1.0, 3.0]), ([9], [1.0])]
    ds = DataSet.from_pairs(pref, oth, batch_rows=3)
    assert ds.size == 6 and ds.batch_rows == 4                      # an odd batch_rows would cut a pair
    assert ds.y.tolist() == [1.0, 0.0, 1.0, 0.0, 1.0, 0.0]
    assert ds.row_ptr.tolist() == [0, 2, 3, 4, 7, 7, 8]
    assert ds.col.tolist() == [1, 5, 3, 2, 4, 6, 7, 9]
    assert ds.val.tolist() == [1.0, 0.5, 0.25, 2.0, 1.0, 1.0, 3.0, 1.0]
    # from_rows' own form, (label, (indices, values)): the labels are ignored
    ds2 = DataSet.from_pairs([(7.0, p) for p in pref], [(-3.0, o) for o in oth], batch_rows=4)
    assert ds2.batch_rows == 4 and ds2.y.tolist() == ds.y.tolist()
    assert ds2.row_ptr.tolist() == ds.row_ptr.tolist() and ds2.col.tolist() == ds.col.tolist() and ds2.val.tolist() == ds.val.tolist()
    assert DataSet.from_pairs(pref, oth).batch_rows == 0            # one batch stays one batch
    with pytest.raises(ValueError, match="equally long"):
        DataSet.from_pairs(pref, oth[:2])
    e = DataSet.from_pairs([], [])
    assert e.size == 0


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_reference_g_is_the_derivative_of_the_pair_loss(loss):
    """train_ref.pair_g against a central difference of train_ref.pair_loss in d, at ordinary and at saturated margins, for
    targets of both signs and ties.  Bound of the difference quotient with step h: h^2/6 * max|loss'''| (<= 0.1 for the
    logistic loss, 0 for the squared one) + 2 eps * max|loss| / h."""
    d = np.array([-40.0, -12.5, -3.0, -0.7, -1e-3, 0.0, 1e-3, 0.4, 2.0, 9.0, 40.0])
    h = 1e-4
    for dy in (1.0, -1.0, 0.0, 2.0):
        dyv = np.full(len(d), dy)
        lo, hi = train_ref.pair_loss(d - h, dyv, loss), train_ref.pair_loss(d + h, dyv, loss)
        fd = (hi - lo) / (2 * h)
        tol = h * h / 6 * 0.1 + 2 * np.finfo(np.float64).eps * np.maximum(np.abs(lo), np.abs(hi)).max() / h
        g = train_ref.pair_g(d, dyv, loss)
        assert np.abs(g - fd).max() <= tol, (dy, np.abs(g - fd).max(), tol)
    if loss == "logistic":
        # a margin saturated on the right side leaves a tiny residual, not a cancelled one
        assert train_ref.pair_g(40.0, 1.0, loss) == pytest.approx(-np.exp(-40.0), rel=1e-12)
        assert train_ref.pair_g(-40.0, -1.0, loss) == pytest.approx(np.exp(-40.0), rel=1e-12)
        # BPR: the preferred row first with the larger label -> -log sigmoid(yhat_preferred - yhat_other)
        assert train_ref.pair_loss(0.3, 1.0, loss) == pytest.approx(-np.log(train_ref.sigmoid(0.3)), rel=1e-14)
        assert train_ref.pair_loss(0.0, 1.0, loss) == pytest.approx(np.log(2.0), rel=1e-15)


def test_reference_residuals_and_scores():
    yh = np.array([0.5, -0.5, 0.0, 0.0, -2.0, 1.0, 3.0, 3.5])
    y = np.array([1.0, 0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0])
    for loss in ("squared", "logistic"):
        e = train_ref.residuals(yh, y, loss, True)
        assert np.array_equal(e[0::2], -e[1::2]) and e.sum() == 0.0
    ll, conc = train_ref.pair_scores(yh, y)
    # pairs: d = 1 (t), 0 (t: a tie), -3 (not t), -0.5 (not t: dy = 0)
    sp = train_ref.softplus
    assert ll == pytest.approx((sp(-1.0) + sp(0.0) + sp(-3.0) + sp(-0.5)) / 4, rel=1e-15)
    assert conc == (1 + 0.5 + 1 + 1) / 4
