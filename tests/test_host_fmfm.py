"""The field-matrixed FM's host surface (no GPU): header against binding, the refusals that need no device, the build's unit list, the
twin on the planted task beside the FM's, the FFM's and the FwFM's."""
import ctypes as C
import os
import re

import numpy as np

import ffm_ref
import fmfm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_matches_the_binding_and_the_build():
    import sparkfm_amd
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_fmfm.h")).read()
    declared = set(re.findall(r"\b(fmhip_fmfm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_FMFM) and len(_ffi.SYMBOLS_FMFM) == 13
    L = _ffi.load()
    for name in _ffi.SYMBOLS_FMFM:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    for name, value in (("FIELDS", _ffi.FMFM_MAX_FIELDS), ("FACTORS", _ffi.FMFM_MAX_FACTORS), ("WIDTH", _ffi.FMFM_MAX_WIDTH)):
        assert int(re.search(r"#define FMHIP_FMFM_MAX_%s (\d+)" % name, hdr).group(1)) == value
    kern = open(os.path.join(ROOT, "sparkfm_amd", "csrc", "fm_fmfm.h")).read()
    for name, value in (("kFmfmRowsPerBlock", _ffi.FMFM_FORWARD_ROWS), ("kFmfmGradRows", _ffi.FMFM_GRAD_ROWS)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, kern).group(1)) == value
    assert {"fm_fmfm.hip", "fmhip_fmfm.hip"} <= set(_build.HIP_SOURCES) and {"fm_fmfm.h", "fm_fwfm.h", "fmhip_ffm_dataset.h"} <= set(_build.HIP_DEPS)
    assert _build.UNIT_FLAGS["fm_fmfm.hip"] == _build.NO_PACKED_FP32
    assert {"FmFM", "FmFMModel", "HipFmFM"} <= set(sparkfm_amd.__all__)


def test_c_calls_refuse_without_a_device():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    err = L.fmhip_last_error
    h = C.c_void_p()
    for call in (lambda: L.fmhip_fmfm_model_info(None, None, None, None, None), lambda: L.fmhip_fmfm_model_set_params(None, 0.0, None, None, None),
                 lambda: L.fmhip_fmfm_model_get_params(None, None, None, None, None), lambda: L.fmhip_fmfm_model_set_rule(None, 0, 0, 1e-10, 1.0),
                 lambda: L.fmhip_fmfm_model_set_linear(None, 1), lambda: L.fmhip_fmfm_model_set_field_matrices(None, 1),
                 lambda: L.fmhip_fmfm_model_get_accumulators(None, None, None, None, None),
                 lambda: L.fmhip_fmfm_model_set_accumulators(None, 0.0, None, None, None), lambda: L.fmhip_fmfm_predict(None, None, None),
                 lambda: L.fmhip_fmfm_step(None, None, 0, 0.1, 0.0, 0.0, 0.0, 0.0, None),
                 lambda: L.fmhip_fmfm_epoch(None, None, 0.1, 0.0, 0.0, 0.0, 0.0, None, None)):
        assert call() == -1 and b"the FmFM model handle is NULL" in err()
    assert L.fmhip_fmfm_model_destroy(None) == 0
    assert L.fmhip_fmfm_model_create(0, 10, 2, 4, None, None) == -1 and b"out is NULL" in err()
    for args, code, msg in (((-1, 2, 4), -1, "num_attribute = -1"), ((10, 0, 4), -1, "num_fields = 0"),
                            ((10, 65, 4), -5, "num_fields = 65 is above FMHIP_FMFM_MAX_FIELDS = 64"), ((10, 2, 0), -1, "num_factor = 0"),
                            ((10, 2, 17), -5, "num_factor = 17 is above FMHIP_FMFM_MAX_FACTORS = 16"),
                            ((10, 64, 16), -5, "F·Kp = 1024 is above 768"), ((10, 49, 9), -5, "F·Kp = 784 is above 768")):
        assert L.fmhip_fmfm_model_create(0, args[0], args[1], args[2], None, C.byref(h)) == code and msg.encode() in err(), args
        assert h.value is None


def test_the_twin_on_the_planted_task():
    """The README's numbers: held-out log-loss of the FmFM twin after 20 epochs of AdaGrad, beside the FM's 0.6212, the FFM's 0.5281 and
    the FwFM's 0.6979.  Every row of the task holds one entry per field, so the twin with M = I frozen is the plain FM's twin: that
    identity (to 1e-12: v^T I v' and <v, v'> round apart) is all that is asserted; the FmFM's own numbers are printed as they come out."""
    t = ref.planted()
    for rows, _ in (t["train"], t["test"]):
        assert all(sorted(f for f, _, _ in row) == list(range(ffm_ref.P_FIELDS)) for row in rows)
    _, fm_train, fm_test_ = ref.run_planted(t, 3)
    frozen, _, frozen_test = ref.run_planted(t, 3, field_matrices=False)
    fm, _, fm_test = ffm_ref.run_planted(t, fm=True)
    print("FmFM: train %.4f test %.4f; FM: test %.4f (README: FM 0.6212, FFM 0.5281, FwFM 0.6979)" % (fm_train, fm_test_, fm_test))
    assert abs(frozen_test - fm_test) <= 1e-12 and np.abs(frozen.v - fm.v[:, 0]).max() <= 1e-12 and np.array_equal(frozen.m, ref.identity(3, ref.P_K))
