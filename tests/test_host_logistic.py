"""The loss selector's host surface (no GPU): argument checks of fmhip_model_set_loss / fmhip_logloss, the learners' `loss=`
and the header's enum against the binding's constants."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_null_model_is_refused():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    assert L.fmhip_model_set_loss(None, _ffi.LOSS_LOGISTIC) == -1
    assert b"NULL" in L.fmhip_last_error()
    r = C.c_double()
    assert L.fmhip_logloss(None, None, C.byref(r), None) == -1
    assert L.fmhip_logloss(None, None, None, None) == -1


def test_unknown_loss_value_is_refused():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    # the value is checked before the handle (a model needs a device): the message names it
    for bad in (7, -1, 2):
        assert L.fmhip_model_set_loss(None, bad) == -1
        assert ("loss %d" % bad).encode() in L.fmhip_last_error()
    with pytest.raises(ValueError, match="hinge"):
        _ffi.loss_code("hinge")
    assert _ffi.loss_code("squared") == 0 and _ffi.loss_code("logistic") == 1


def test_learners_refuse_an_unknown_loss():
    from sparkfm_amd import HipSGD
    from sparkfm_amd.distributed import DataParallelSGD, HipDataParallelSGD
    with pytest.raises(ValueError):
        HipSGD(loss="hinge")
    with pytest.raises(ValueError):
        HipSGD.run(loss="absolute")
    with pytest.raises(ValueError):
        DataParallelSGD(loss="hinge")
    with pytest.raises(ValueError):
        HipDataParallelSGD(None, loss="hinge")     # refused before the communicator is touched
    assert HipSGD(loss="logistic").loss == "logistic" and HipSGD().loss == "squared"


def test_header_enum_matches_the_binding():
    from sparkfm_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip.h")).read()
    m = re.search(r"enum fmhip_loss \{([^}]*)\}", hdr)
    assert m
    vals = dict((k, int(v)) for k, v in re.findall(r"FMHIP_LOSS_([A-Z]+) = (\d+)", m.group(1)))
    assert vals == {"SQUARED": _ffi.LOSS_SQUARED, "LOGISTIC": _ffi.LOSS_LOGISTIC}
    assert {"fmhip_model_set_loss", "fmhip_logloss"} <= set(_ffi.SYMBOLS)
    L = _ffi.load()
    assert hasattr(L, "fmhip_model_set_loss") and hasattr(L, "fmhip_logloss")
