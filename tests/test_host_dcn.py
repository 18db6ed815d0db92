"""The cross network's host surface (no GPU): header against binding and build, the refusals that need no device, the twin's gradient
against central differences, the L = 1 identity with the FmFM's form, the twin on the planted task beside the family's numbers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dcn_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_matches_the_binding_and_the_build():
    import sparkfm_amd
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_dcn.h")).read()
    declared = set(re.findall(r"\b(fmhip_dcn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_DCN) and len(_ffi.SYMBOLS_DCN) == 13
    L = _ffi.load()
    for name in _ffi.SYMBOLS_DCN:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    for name in ("FIELDS", "FACTORS", "WIDTH", "LAYERS", "RANK"):
        assert int(re.search(r"#define FMHIP_DCN_MAX_%s (\d+)" % name, hdr).group(1)) == getattr(_ffi, "DCN_MAX_" + name)
    kern = open(os.path.join(ROOT, "sparkfm_amd", "csrc", "fm_dcn.h")).read()
    for name, value in (("kDcnRowsPerBlock", _ffi.DCN_FORWARD_ROWS), ("kDcnGradRows", _ffi.DCN_GRAD_ROWS)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, kern).group(1)) == value
    assert {"fm_dcn.hip", "fmhip_dcn.hip"} <= set(_build.HIP_SOURCES) and "fm_dcn.h" in _build.HIP_DEPS
    assert _build.UNIT_FLAGS["fm_dcn.hip"] == _build.NO_PACKED_FP32
    assert {"DCN", "DCNModel", "HipDCN"} <= set(sparkfm_amd.__all__)


@pytest.mark.parametrize("shape,layers,rank,code,msg", [
    ((10, 0, 4), 1, 16, -1, "num_fields = 0"), ((10, 65, 4), 1, 16, -5, "num_fields = 65"),
    ((10, 2, 0), 1, 16, -1, "num_factor = 0"), ((10, 2, 17), 1, 16, -5, "num_factor = 17"),
    ((10, 49, 9), 1, 16, -5, "F·Kp = 784 is above 768"),
    ((10, 2, 4), 0, 16, -1, "n_layers = 0"), ((10, 2, 4), 4, 16, -5, "n_layers = 4 is above FMHIP_DCN_MAX_LAYERS = 3"),
    ((10, 2, 4), 1, 0, -1, "rank = 0"), ((10, 2, 4), 1, 24, -1, "rank = 24"), ((10, 2, 4), 1, 272, -5, "rank = 272 is above FMHIP_DCN_MAX_RANK = 256")])
def test_create_refuses_without_a_device(shape, layers, rank, code, msg):
    from sparkfm_amd import _ffi
    L, h = _ffi.load(), C.c_void_p()
    assert L.fmhip_dcn_model_create(0, shape[0], shape[1], shape[2], layers, rank, None, C.byref(h)) == code
    assert msg.encode() in L.fmhip_last_error() and h.value is None


def small(seed=5, F=3, k=2, L=2, r=16, n1=12, fields=None):
    rng = np.random.default_rng(seed)
    rows = ref.random_rows(rng, 5, n1, F, [3, 4, 2, 5, 3], one_field_row=False)
    if fields is not None:
        rows = [[(fields[f % len(fields)], i, x) for f, i, x in row] for row in rows]
    cross, u = ref.dense(rng, F, k, L, r, c_std=0.3)
    return ref.State(0.3, rng.normal(0, 0.3, n1), rng.normal(0, 0.3, (n1, k)), cross, u), rows, rng.normal(0, 1, 5)


def flat(G):
    return np.concatenate([np.ravel(G["w0"]), G["w"].ravel(), G["v"].ravel()] + [x.ravel() for t in G["cross"] for x in t] + [G["u"]])


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_the_twins_gradient_against_central_differences(loss):
    """F = 3, k = 2, L = 2, r = 16, 5 rows; every parameter.  The loss is a polynomial of degree <= 2 (L + 2) in any one parameter
    (under the logistic loss: composed with a smooth function), so the central difference's truncation error falls as h^2 and its
    rounding error grows as 1e-16 / h.  Measured, the worst |difference| / (1 + |g|) under the squared (logistic) loss is 2.50e-7
    (8.5e-8) at h = 1e-3, 2.50e-9 (8.5e-10) at 1e-4, 2.7e-11 (1.2e-11) at 1e-5 — still the h^2 law, and the minimum — then 7.9e-11
    (1.2e-10) at 1e-6 and 7.4e-10 (1.2e-9) at 1e-7, the rounding branch.  h = 1e-5 is used, and the tolerance is 1e-10 (1 + |g|): the
    h^2 law's 2.5e-11 plus the rounding branch's 1e-16 / h = 1e-11 each with a factor 3 (worst ratio measured: 0.27 and 0.12).  A
    wrong term in the chain rule is an error of the order of the gradient itself, |g| up to 0.6 here.  Also: a field no row holds has x_0 = 0 on its slots, and the gradient of V_l's rows, U_l's columns,
    c_l and u there is exactly 0 — what keeps the device's pad slots at 0."""
    s, rows, y = small()
    g = flat(ref.gradients(s, rows, y, loss))

    def value():
        yh = ref.predict(s, rows)[0]
        return float(np.mean(0.5 * (yh - y) ** 2 if loss == "squared" else np.maximum(yh, 0.0) - (y > 0) * yh + np.log1p(np.exp(-np.abs(yh)))))

    arrays = [s.w, s.v] + [x for t in s.cross for x in t] + [s.u]
    h, fd = 1e-5, []
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
    ratio = np.abs(np.array(fd) - g) / (1e-10 * (1 + np.abs(g)))
    print("worst |fd - g| / tol %.3f" % ratio.max())
    assert ratio.max() <= 1.0
    s2, rows2, y2 = small(fields=[0, 1])
    G, k = ref.gradients(s2, rows2, y2, loss), 2
    for gV, gU, gc in G["cross"]:
        assert not gV[2 * k:].any() and not gU[:, 2 * k:].any() and not gc[2 * k:].any() and gV[:2 * k].any() and gU[:, :2 * k].any()
    assert not G["u"][2 * k:].any() and G["u"][:2 * k].any()


def test_one_layer_with_c_minus_one_and_u_one_is_the_fmfm_form():
    """L = 1, c = -1, u = 1: x_1 = s o (s V U - 1) + s = s o (s V U), so the cross term is s^T (V_0 U_0) s, to 1e-12."""
    s, rows, _ = small(seed=6, L=1)
    (V, U, c), k = s.cross[0], s.v.shape[1]
    s.cross, s.u = [(V, U, np.full_like(c, -1.0))], np.ones_like(s.u)
    s.w0, s.w = 0.0, np.zeros_like(s.w)
    yh = ref.predict(s, rows)[0]
    for r, row in enumerate(rows):
        sums = np.zeros(len(s.u))
        for f, i, x in row:
            sums[f * k:(f + 1) * k] += x * s.v[i]
        assert abs(yh[r] - sums @ (V @ U) @ sums) <= 1e-12 * max(1.0, abs(yh[r]))


def test_the_twin_on_the_planted_task():
    """The README's number: held-out log-loss of the DCN twin, two cross layers of rank 16, after 20 epochs of AdaGrad, beside the FM's
    0.6212, the FFM's 0.5281, the FwFM's 0.6979, the FmFM's 0.6347 and DeepFM's 0.9051; printed as it comes out."""
    t = ref.planted()
    _, train, test = ref.run_planted(t)
    print("DCN: train %.4f test %.4f (README: FM 0.6212, FFM 0.5281, FwFM 0.6979, FmFM 0.6347, DeepFM 0.9051)" % (train, test))
    assert np.isfinite(train) and np.isfinite(test)
