"""The CIN's host surface (no GPU): header against binding and build, the refusals that need no device, the twin's gradient against
central differences, the one-layer closed form."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cin_ref as ref
from test_host_field_models import test_c_calls_refuse_without_a_device as shared_refusals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_matches_the_binding_and_the_build():
    import sparkfm_amd
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_cin.h")).read()
    declared = set(re.findall(r"\b(fmhip_cin_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_CIN) and len(_ffi.SYMBOLS_CIN) == 13
    L = _ffi.load()
    for name in _ffi.SYMBOLS_CIN:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    for name in ("FIELDS", "FACTORS", "LAYERS", "MAPS"):
        assert int(re.search(r"#define FMHIP_CIN_MAX_%s (\d+)" % name, hdr).group(1)) == getattr(_ffi, "CIN_MAX_" + name)
    kern = open(os.path.join(ROOT, "sparkfm_amd", "csrc", "fm_cin.h")).read()
    assert int(re.search(r"constexpr int kCinRowsPerBlock = (\d+);", kern).group(1)) == _ffi.CIN_FORWARD_ROWS
    assert int(re.search(r"constexpr int kCinGradRows = (\d+);", kern).group(1)) == _ffi.CIN_GRAD_ROWS
    assert {"fm_cin.hip", "fmhip_cin.hip"} <= set(_build.HIP_SOURCES) and "fm_cin.h" in _build.HIP_DEPS
    assert _build.UNIT_FLAGS["fm_cin.hip"] == _build.NO_PACKED_FP32
    assert {"CIN", "CINModel", "HipCIN"} <= set(sparkfm_amd.__all__)


@pytest.mark.parametrize("k,maps,code,msg", [
    (4, (), -1, "n_layers = 0"), (4, (16, 16, 16, 16), -5, "n_layers = 4 is above FMHIP_CIN_MAX_LAYERS = 3"),
    (4, (8,), -1, "feature_maps[0] = 8"), (4, (16, 24), -1, "feature_maps[1] = 24"), (4, (144,), -5, "feature_maps[0] = 144 is above FMHIP_CIN_MAX_MAPS = 128"),
    (17, (16,), -5, "num_factor = 17 is above FMHIP_CIN_MAX_FACTORS = 16")])
def test_create_refuses_without_a_device(k, maps, code, msg):
    from sparkfm_amd import _ffi
    L, h = _ffi.load(), C.c_void_p()
    assert L.fmhip_cin_model_create(0, 10, 2, k, len(maps), (C.c_int32 * max(len(maps), 1))(*maps), None, C.byref(h)) == code
    assert msg.encode() in L.fmhip_last_error() and h.value is None


def test_the_shared_refusals():
    shared_refusals("CIN", "CIN", "cin", "set_cin", 2, 2, lambda: (1, (C.c_int32 * 1)(16)))


def small(seed=5, F=3, k=2, maps=(16, 16), n1=12):
    rng = np.random.default_rng(seed)
    rows = ref.random_rows(rng, 5, n1, F, [3, 4, 2, 5, 3], one_field_row=False)
    layers, u = ref.dense(rng, F, k, maps)
    return ref.State(0.3, rng.normal(0, 0.3, n1), rng.normal(0, 0.3, (n1, k)), layers, u), rows, rng.normal(0, 1, 5)


H_STEP, FD_TOL = 1e-5, 5.3e-11


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_the_twins_gradient_against_central_differences(loss):
    """F = 3, k = 2, maps (16, 16), 5 rows; every parameter.  The model is a polynomial in its parameters, so there is no kink to guard:
    the central difference's truncation error falls as h^2 and its rounding error grows as 1e-16 / h.  Measured, the worst
    |difference| / (1 + |g|) under the squared (logistic) loss is 7.70e-8 (2.95e-8) at h = 1e-3, 7.70e-10 (2.94e-10) at 1e-4, 1.35e-11
    (1.15e-11) at 1e-5 — the minimum, where the two branches meet — then 1.43e-10 (1.29e-10) at 1e-6 and 1.44e-9 (1.09e-9) at 1e-7, the
    rounding branch.  h = 1e-5 is used, and the tolerance is 5.3e-11 (1 + |g|): the h^2 law's 7.7e-12 plus the rounding branch's
    1e-16 / h = 1e-11, each with a factor 3 (|g| up to 0.29 here).  A wrong term in the chain rule is an error of the order of the
    gradient itself."""
    s, rows, y = small()
    G = ref.gradients(s, rows, y, loss)
    g = np.concatenate([np.ravel(G["w0"]), G["w"].ravel(), G["v"].ravel()] + [x.ravel() for x in G["layers"]] + [G["u"]])

    def value():
        yh = ref.predict(s, rows)[0]
        return float(np.mean(0.5 * (yh - y) ** 2 if loss == "squared" else np.maximum(yh, 0.0) - (y > 0) * yh + np.log1p(np.exp(-np.abs(yh)))))

    h, fd = H_STEP, []
    for sign in (1, -1):
        s.w0 += sign * h
        fd.append(value())
        s.w0 -= sign * h
    fd = [(fd[0] - fd[1]) / (2 * h)]
    for a in [s.w, s.v] + s.layers + [s.u]:
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


def test_one_layer_is_the_field_weighted_form():
    """L = 1, u = e_0, W_1[0] = R: the CIN term is sum_{i,j} R_ij <S_i, S_j>, to 1e-12."""
    s, rows, _ = small(seed=6, maps=(16,))
    s.u[:] = 0.0
    s.u[0] = 1.0
    R, k = s.layers[0][0], s.v.shape[1]
    lin = ref.State(s.w0, s.w, s.v, s.layers, np.zeros_like(s.u))
    got = ref.predict(s, rows)[0] - ref.predict(lin, rows)[0]
    for r, row in enumerate(rows):
        S = np.zeros((R.shape[0], k))
        for f, i, x in row:
            S[f] += x * s.v[i]
        assert abs(got[r] - (R * (S @ S.T)).sum()) <= 1e-12
