"""The AFM's host surface (no GPU): header against binding and build, the refusals that need no device, the twin's gradient against
central differences, the one-field model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import afm_ref as ref
from test_host_field_models import test_c_calls_refuse_without_a_device as shared_refusals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_matches_the_binding_and_the_build():
    import sparkfm_amd
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_afm.h")).read()
    declared = set(re.findall(r"\b(fmhip_afm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_AFM) and len(_ffi.SYMBOLS_AFM) == 13
    L = _ffi.load()
    for name in _ffi.SYMBOLS_AFM:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    for name in ("FIELDS", "FACTORS", "ATTENTION"):
        assert int(re.search(r"#define FMHIP_AFM_MAX_%s (\d+)" % name, hdr).group(1)) == getattr(_ffi, "AFM_MAX_" + name)
    kern = open(os.path.join(ROOT, "sparkfm_amd", "csrc", "fm_afm.h")).read()
    assert int(re.search(r"constexpr int kAfmRowsPerBlock = (\d+);", kern).group(1)) == _ffi.AFM_FORWARD_ROWS
    assert {"fm_afm.hip", "fmhip_afm.hip"} <= set(_build.HIP_SOURCES) and "fm_afm.h" in _build.HIP_DEPS
    assert _build.UNIT_FLAGS["fm_afm.hip"] == _build.NO_PACKED_FP32
    assert {"AFM", "AFMModel", "HipAFM"} <= set(sparkfm_amd.__all__)


@pytest.mark.parametrize("k,t,code,msg", [
    (4, 0, -1, "attention_factor = 0"), (4, 8, -1, "attention_factor = 8"), (4, 24, -1, "attention_factor = 24"),
    (4, 80, -5, "attention_factor = 80 is above FMHIP_AFM_MAX_ATTENTION = 64"), (17, 16, -5, "num_factor = 17 is above FMHIP_AFM_MAX_FACTORS = 16")])
def test_create_refuses_without_a_device(k, t, code, msg):
    from sparkfm_amd import _ffi
    L, h = _ffi.load(), C.c_void_p()
    assert L.fmhip_afm_model_create(0, 10, 2, k, t, None, C.byref(h)) == code
    assert msg.encode() in L.fmhip_last_error() and h.value is None


def test_the_shared_refusals():
    shared_refusals("AFM", "AFM", "afm", "set_attention", 4, 1, lambda: (16,))


def small(seed=5, F=4, k=2, t=16, n1=12):
    rng = np.random.default_rng(seed)
    rows = ref.random_rows(rng, 5, n1, F, [3, 4, 2, 5, 3], one_field_row=False)
    return ref.State(0.3, rng.normal(0, 0.3, n1), rng.normal(0, 1.0, (n1, k)), *ref.dense(rng, k, t)), rows, rng.normal(0, 1, 5)


H_STEP, FD_TOL = 1e-5, 3.4e-11


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_the_twins_gradient_against_central_differences(loss):
    """F = 4, k = 2, t = 16, 5 rows; every parameter.  Asserted first: no unit's pre-activation is within 1e-3 of the kink, a hundred
    steps h away, so both evaluations of a difference see the masks the gradient was taken with and the model is smooth between them.
    The central difference's truncation error falls as h^2 and its rounding error grows as 1e-16 / h.  Measured, the worst
    |difference| / (1 + |g|) under the squared (logistic) loss is 1.07e-8 (1.23e-8) at h = 1e-3, 1.07e-10 (1.23e-10) at 1e-4, 8.33e-12
    (7.86e-12) at 1e-5 — the minimum, where the two branches meet — then 8.33e-11 (9.9e-11) at 1e-6 and 9.97e-10 (7.97e-10) at 1e-7, the
    rounding branch.  h = 1e-5 is used, and the tolerance is 3.4e-11 (1 + |g|): the h^2 law's 1.23e-12 plus the rounding branch's
    1e-16 / h = 1e-11, each with a factor 3 (|g| up to 0.36 here; the smallest |pre-activation| is 2.2e-3).  A wrong term in the chain
    rule is an error of the order of the gradient itself."""
    s, rows, y = small()
    G = ref.gradients(s, rows, y, 4, loss)
    assert G["margin"] >= 1e-3
    arrays = [s.w, s.v] + [getattr(s, name) for name in ref.DENSE]
    g = np.concatenate([np.ravel(G["w0"]), G["w"].ravel(), G["v"].ravel()] + [G[name].ravel() for name in ref.DENSE])

    def value():
        yh = ref.predict(s, rows, 4)[0]
        return float(np.mean(0.5 * (yh - y) ** 2 if loss == "squared" else np.maximum(yh, 0.0) - (y > 0) * yh + np.log1p(np.exp(-np.abs(yh)))))

    h, fd = H_STEP, []
    for sign in (1, -1):
        s.w0 += sign * h
        fd.append(value())
        s.w0 -= sign * h
    fd = [(fd[0] - fd[1]) / (2 * h)]
    for a in arrays:
        for idx in np.ndindex(a.shape):
            keep = a[idx]
            a[idx] = keep + h
            up = value()
            a[idx] = keep - h
            fd.append((up - value()) / (2 * h))
            a[idx] = keep
    ratio = np.abs(np.array(fd) - g) / (FD_TOL * (1 + np.abs(g)))
    print("worst |fd - g| / tol %.3f" % ratio.max())
    assert ratio.max() <= 1.0


def test_one_field_scores_as_the_linear_model():
    """F = 1: no pair, the AFM term is 0 and the attention part's gradient is 0."""
    s, _, y = small()
    rows = ref.random_rows(np.random.default_rng(2), 5, 12, 1, [3, 4, 2, 5, 3], one_field_row=False)
    yh, _, bound = ref.predict(s, rows, 1)
    assert np.array_equal(yh, [sum((s.w[i] * x for _, i, x in row), s.w0) for row in rows]) and not bound.any()
    G = ref.gradients(s, rows, y, 1)
    assert not any(G[name].any() for name in ref.DENSE) and not G["v"].any()
