"""The PNN's host surface (no GPU): header against binding and build, the refusals that need no device, the twin's gradient against
central differences, the one-field model."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pnn_ref as ref
from test_host_field_models import test_c_calls_refuse_without_a_device as shared_refusals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_matches_the_binding_and_the_build():
    import sparkfm_amd
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_pnn.h")).read()
    declared = set(re.findall(r"\b(fmhip_pnn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_PNN) and len(_ffi.SYMBOLS_PNN) == 13
    L = _ffi.load()
    for name in _ffi.SYMBOLS_PNN:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    for name in ("FIELDS", "FACTORS", "LAYERS", "UNITS", "WIDTH"):
        assert int(re.search(r"#define FMHIP_PNN_MAX_%s (\d+)" % name, hdr).group(1)) == getattr(_ffi, "PNN_MAX_" + name)
    kern = open(os.path.join(ROOT, "sparkfm_amd", "csrc", "fm_pnn.h")).read()
    assert int(re.search(r"constexpr int kPnnRowsPerBlock = (\d+);", kern).group(1)) == _ffi.PNN_FORWARD_ROWS
    assert {"fm_pnn.hip", "fmhip_pnn.hip"} <= set(_build.HIP_SOURCES) and "fm_pnn.h" in _build.HIP_DEPS
    assert any(d.endswith("fmhip_pnn.h") for d in _build.HIP_DEPS) and _build.UNIT_FLAGS["fm_pnn.hip"] == _build.NO_PACKED_FP32
    assert {"PNN", "PNNModel", "HipPNN"} <= set(sparkfm_amd.__all__)


@pytest.mark.parametrize("F,k,widths,code,msg", [
    (50, 4, (16,), -5, "= 208 + 1232 = 1440 is above FMHIP_PNN_MAX_WIDTH = 1408"), (40, 16, (16,), -5, "= 640 + 784 = 1424 is above"),
    (2, 17, (16,), -5, "num_factor = 17 is above FMHIP_PNN_MAX_FACTORS = 16"), (2, 4, (), -1, "n_layers = 0"),
    (2, 4, (16,) * 4, -5, "n_layers = 4 is above FMHIP_PNN_MAX_LAYERS = 3"), (2, 4, (16, 8), -1, "widths[1] = 8"), (2, 4, (24,), -1, "widths[0] = 24"),
    (2, 4, (272,), -5, "widths[0] = 272 is above FMHIP_PNN_MAX_UNITS = 256")])
def test_create_refuses_without_a_device(F, k, widths, code, msg):
    from sparkfm_amd import _ffi
    L, h = _ffi.load(), C.c_void_p()
    assert L.fmhip_pnn_model_create(0, 10, F, k, len(widths), (C.c_int32 * max(len(widths), 1))(*widths), None, C.byref(h)) == code
    assert msg.encode() in L.fmhip_last_error() and h.value is None


def test_the_shared_refusals():
    shared_refusals("PNN", "PNN", "pnn", "set_deep", 3, 2, lambda: (1, (C.c_int32 * 1)(16)))


def small(seed=5, F=4, k=2, n1=12):
    rng = np.random.default_rng(seed)
    rows = ref.random_rows(rng, 5, n1, F, [3, 4, 2, 5, 3], one_field_row=False)
    layers, u = ref.dense(rng, F, k, (16,))
    layers = [(W, rng.normal(0, 1, len(b))) for W, b in layers]
    return ref.State(0.3, rng.normal(0, 0.3, n1), rng.normal(0, 1.0, (n1, k)), layers, u), rows, rng.normal(0, 1, 5)


H_STEP, FD_TOL = 1e-5, 4.3e-11


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_the_twins_gradient_against_central_differences(loss):
    """F = 4, k = 2, hidden (16,), 5 rows; every parameter.  Asserted first: no unit's pre-activation is within 1e-3 of the kink, a
    hundred steps h away (the smallest here is 3.1e-2), so both evaluations of a difference see the masks the gradient was taken with.
    The central difference's truncation error falls as h^2 and its rounding error grows as 1e-16 / h.  Measured, the worst
    |difference| / (1 + |g|) under the logistic loss is 4.22e-8 at h = 1e-3, 4.22e-10 at 1e-4, 7.29e-12 at 1e-5 — where the two branches
    meet —, then 6.34e-11 at 1e-6 and 7.41e-10 at 1e-7, the rounding branch; under the squared loss (a polynomial of low degree between
    the kinks: next to no truncation) 1.8e-14, 3.5e-13, 1.29e-12, 1.60e-11, 1.79e-10.  h = 1e-5 is used, and the tolerance is
    4.3e-11 (1 + |g|): the h^2 law's 4.22e-12 plus the rounding branch's 1e-16 / h = 1e-11, each with a factor 3 (|g| up to 0.43 here).
    A wrong term in the chain rule is an error of the order of the gradient itself."""
    s, rows, y = small()
    assert ref.margin(s, rows) >= 1e-3
    G = ref.gradients(s, rows, y, loss)
    arrays = [s.w, s.v, s.layers[0][0], s.layers[0][1], s.u]
    g = np.concatenate([np.ravel(G["w0"]), G["w"].ravel(), G["v"].ravel(), G["layers"][0][0].ravel(), G["layers"][0][1].ravel(), G["u"].ravel()])

    def value():
        yh = ref.predict(s, rows)[0]
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
    worst = (np.abs(np.array(fd) - g) / (1 + np.abs(g))).max()
    print("worst |fd - g| / (1 + |g|) %.3g, / tol %.3f" % (worst, worst / max(FD_TOL, 1e-300)))
    assert worst <= FD_TOL


def test_one_field_scores_as_the_mlp_over_s():
    """F = 1: no pair, G = 0, W_1 is k x n_1 and the model is an MLP over the row's one field sum."""
    rng = np.random.default_rng(3)
    rows = ref.random_rows(rng, 5, 12, 1, [3, 4, 2, 5, 3], one_field_row=False)
    layers, u = ref.dense(rng, 1, 2, (16,))
    s = ref.State(0.3, rng.normal(0, 0.3, 12), rng.normal(0, 1.0, (12, 2)), layers, u)
    assert s.layers[0][0].shape == (2, 16) and ref.fields(s) == 1
    want = [s.w0 + sum(s.w[i] * x for _, i, x in row) + np.maximum(sum(x * s.v[i] for _, i, x in row) @ s.layers[0][0], 0.0) @ s.u for row in rows]
    assert np.allclose(ref.predict(s, rows)[0], want, rtol=1e-14, atol=0)
