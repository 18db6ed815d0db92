"""The field-weighted FM's host surface (no GPU): header against binding, the refusals that need no device, the build's unit list, the
twin on the planted task beside the FFM's and the plain FM's."""
import ctypes as C
import os
import re

import numpy as np

import ffm_ref
import fwfm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_matches_the_binding_and_the_build():
    import sparkfm_amd
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_fwfm.h")).read()
    declared = set(re.findall(r"\b(fmhip_fwfm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_FWFM) and len(_ffi.SYMBOLS_FWFM) == 13
    L = _ffi.load()
    for name in _ffi.SYMBOLS_FWFM:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    for name, value in (("FIELDS", _ffi.FWFM_MAX_FIELDS), ("FACTORS", _ffi.FWFM_MAX_FACTORS)):
        assert int(re.search(r"#define FMHIP_FWFM_MAX_%s (\d+)" % name, hdr).group(1)) == value
    assert {"fm_fwfm.hip", "fmhip_fwfm.hip"} <= set(_build.HIP_SOURCES) and {"fm_fwfm.h", "fmhip_ffm_dataset.h"} <= set(_build.HIP_DEPS)
    assert _build.UNIT_FLAGS["fm_fwfm.hip"] == _build.NO_PACKED_FP32
    assert {"FwFM", "FwFMModel", "HipFwFM"} <= set(sparkfm_amd.__all__)


def test_c_calls_refuse_without_a_device():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    err = L.fmhip_last_error
    h = C.c_void_p()
    for call in (lambda: L.fmhip_fwfm_model_info(None, None, None, None, None), lambda: L.fmhip_fwfm_model_set_params(None, 0.0, None, None, None),
                 lambda: L.fmhip_fwfm_model_get_params(None, None, None, None, None), lambda: L.fmhip_fwfm_model_set_rule(None, 0, 0, 1e-10, 1.0),
                 lambda: L.fmhip_fwfm_model_set_linear(None, 1), lambda: L.fmhip_fwfm_model_set_field_weights(None, 1),
                 lambda: L.fmhip_fwfm_model_get_accumulators(None, None, None, None, None),
                 lambda: L.fmhip_fwfm_model_set_accumulators(None, 0.0, None, None, None), lambda: L.fmhip_fwfm_predict(None, None, None),
                 lambda: L.fmhip_fwfm_step(None, None, 0, 0.1, 0.0, 0.0, 0.0, 0.0, None),
                 lambda: L.fmhip_fwfm_epoch(None, None, 0.1, 0.0, 0.0, 0.0, 0.0, None, None)):
        assert call() == -1 and b"the FwFM model handle is NULL" in err()
    assert L.fmhip_fwfm_model_destroy(None) == 0
    assert L.fmhip_fwfm_model_create(0, 10, 2, 4, None, None) == -1 and b"out is NULL" in err()
    for args, code, msg in (((-1, 2, 4), -1, b"num_attribute = -1"), ((10, 0, 4), -1, b"num_fields = 0"),
                            ((10, 65, 4), -5, b"num_fields = 65 is above FMHIP_FWFM_MAX_FIELDS = 64"), ((10, 2, 0), -1, b"num_factor = 0"),
                            ((10, 2, 33), -5, b"num_factor = 33 is above FMHIP_FWFM_MAX_FACTORS = 32")):
        assert L.fmhip_fwfm_model_create(0, args[0], args[1], args[2], None, C.byref(h)) == code and msg in err(), args
        assert h.value is None


def test_the_twin_on_the_planted_task():
    """The README's numbers: held-out log-loss of the FwFM, FFM and plain-FM twins after 20 epochs of AdaGrad.  The planted truth gives
    every feature an independent vector per partner field, which one vector and a scalar per field pair cannot follow: the FwFM twin fits
    the training rows (0.2265) and does NOT beat the plain FM held out (0.6979 against 0.6212; FFM 0.5281).  Asserted, therefore, is only
    that the twin with r = 1 frozen is the plain FM's twin."""
    t = ref.planted()
    _, fw_train, fw_test = ref.run_planted(t, 3)
    frozen, _, frozen_test = ref.run_planted(t, 3, field_weights=False)
    fm, _, fm_test = ffm_ref.run_planted(t, fm=True)
    print("FwFM: train %.4f test %.4f; FFM: test %.4f; FM: test %.4f" % (fw_train, fw_test, ffm_ref.run_planted(t)[2], fm_test))
    assert frozen_test == fm_test and np.array_equal(frozen.v, fm.v[:, 0]) and np.array_equal(frozen.r, np.ones((3, 3)))
