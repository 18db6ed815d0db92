"""DeepFM's host surface (no GPU): header against binding and build, the refusals that need no device, the twin on the planted task
beside the FM's, the FFM's, the FwFM's and the FmFM's."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import deepfm_ref as ref
import fwfm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_matches_the_binding_and_the_build():
    import sparkfm_amd
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_deepfm.h")).read()
    declared = set(re.findall(r"\b(fmhip_deepfm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_DEEPFM) and len(_ffi.SYMBOLS_DEEPFM) == 13
    L = _ffi.load()
    for name in _ffi.SYMBOLS_DEEPFM:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    for name in ("FIELDS", "FACTORS", "WIDTH", "LAYERS", "UNITS"):
        assert int(re.search(r"#define FMHIP_DEEPFM_MAX_%s (\d+)" % name, hdr).group(1)) == getattr(_ffi, "DEEPFM_MAX_" + name)
    kern = open(os.path.join(ROOT, "sparkfm_amd", "csrc", "fm_deepfm.h")).read()
    for name, value in (("kDeepRowsPerBlock", _ffi.DEEPFM_FORWARD_ROWS), ("kDeepGradRows", _ffi.DEEPFM_GRAD_ROWS)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, kern).group(1)) == value
    assert {"fm_deepfm.hip", "fmhip_deepfm.hip"} <= set(_build.HIP_SOURCES) and "fm_deepfm.h" in _build.HIP_DEPS
    assert _build.UNIT_FLAGS["fm_deepfm.hip"] == _build.NO_PACKED_FP32
    assert {"DeepFM", "DeepFMModel", "HipDeepFM"} <= set(sparkfm_amd.__all__)


@pytest.mark.parametrize("shape,widths,code,msg", [
    ((10, 2, 4), [24], -1, "widths[0] = 24"), ((10, 2, 4), [64, 272], -5, "widths[1] = 272 is above FMHIP_DEEPFM_MAX_UNITS = 256"),
    ((10, 2, 4), [16, 0], -1, "widths[1] = 0"), ((10, 2, 4), [16, 16, 16, 16], -5, "n_layers = 4 is above FMHIP_DEEPFM_MAX_LAYERS = 3"),
    ((10, 49, 9), [16], -5, "F·Kp = 784 is above 768"), ((10, 65, 4), [16], -5, "num_fields = 65"), ((10, 2, 17), [16], -5, "num_factor = 17"),
    ((10, 2, 4), [], -1, "n_layers = 0")])
def test_create_refuses_without_a_device(shape, widths, code, msg):
    from sparkfm_amd import _ffi
    L, h = _ffi.load(), C.c_void_p()
    w = (C.c_int32 * max(len(widths), 1))(*widths)
    assert L.fmhip_deepfm_model_create(0, shape[0], shape[1], shape[2], len(widths), w, None, C.byref(h)) == code
    assert msg.encode() in L.fmhip_last_error() and h.value is None


def test_the_twin_on_the_planted_task():
    """The README's number: held-out log-loss of the DeepFM twin, hidden (64, 32), after 20 epochs of AdaGrad, beside the FM's 0.6212, the
    FFM's 0.5281, the FwFM's 0.6979 and the FmFM's 0.6347; printed as it comes out.  Asserted: with u = 0 and the dense part frozen the
    twin is the FwFM's twin with r = 1 frozen (the plain FM over a row's entries), to rounding."""
    t = ref.planted()
    _, train, test = ref.run_planted(t)
    frozen, _, frozen_test = ref.run_planted(t, deep=False, zero_u=True)
    fw, _, fw_test = fwfm_ref.run_planted(t, ref.P_FIELDS, field_weights=False)
    print("DeepFM: train %.4f test %.4f; u = 0, frozen: test %.4f (README: FM 0.6212, FFM 0.5281, FwFM 0.6979, FmFM 0.6347)" % (train, test, frozen_test))
    assert abs(frozen_test - fw_test) <= 1e-12 and np.abs(frozen.v - fw.v).max() <= 1e-12 and not frozen.u.any()
