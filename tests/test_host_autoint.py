"""AutoInt's host surface (no GPU): header against binding and build, the refusals that need no device, the twin's gradient against
central differences, the uniform attention's closed form."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import autoint_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_matches_the_binding_and_the_build():
    import sparkfm_amd
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_autoint.h")).read()
    declared = set(re.findall(r"\b(fmhip_autoint_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_AUTOINT) and len(_ffi.SYMBOLS_AUTOINT) == 13
    L = _ffi.load()
    for name in _ffi.SYMBOLS_AUTOINT:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    for name in ("FIELDS", "FACTORS", "LAYERS", "HEADS", "HEAD_DIM", "WIDTH"):
        assert int(re.search(r"#define FMHIP_AUTOINT_MAX_%s (\d+)" % name, hdr).group(1)) == getattr(_ffi, "AUTOINT_MAX_" + name)
    kern = open(os.path.join(ROOT, "sparkfm_amd", "csrc", "fm_autoint.h")).read()
    assert int(re.search(r"constexpr int kAutoIntRowsPerBlock = (\d+);", kern).group(1)) == _ffi.AUTOINT_FORWARD_ROWS
    assert {"fm_autoint.hip", "fmhip_autoint.hip"} <= set(_build.HIP_SOURCES) and "fm_autoint.h" in _build.HIP_DEPS
    assert _build.UNIT_FLAGS["fm_autoint.hip"] == _build.NO_PACKED_FP32
    assert {"AutoInt", "AutoIntModel", "HipAutoInt"} <= set(sparkfm_amd.__all__)


@pytest.mark.parametrize("shape,lhd,code,msg", [
    ((10, 0, 4), (1, 1, 16), -1, "num_fields = 0"), ((10, 65, 4), (1, 1, 16), -5, "num_fields = 65"),
    ((10, 2, 0), (1, 1, 16), -1, "num_factor = 0"), ((10, 2, 17), (1, 1, 16), -5, "num_factor = 17"),
    ((10, 2, 4), (0, 1, 16), -1, "n_layers = 0"), ((10, 2, 4), (4, 1, 16), -5, "n_layers = 4 is above FMHIP_AUTOINT_MAX_LAYERS = 3"),
    ((10, 2, 4), (1, 0, 16), -1, "heads = 0"), ((10, 2, 4), (1, 3, 16), -1, "heads = 3"), ((10, 2, 4), (1, 8, 16), -5, "heads = 8 is above"),
    ((10, 2, 4), (1, 1, 8), -1, "head_dim = 8"), ((10, 2, 4), (1, 1, 24), -1, "head_dim = 24"), ((10, 2, 4), (1, 1, 64), -5, "head_dim = 64 is above"),
    ((10, 2, 4), (1, 4, 32), -5, "heads·head_dim = 128 is above FMHIP_AUTOINT_MAX_WIDTH = 64")])
def test_create_refuses_without_a_device(shape, lhd, code, msg):
    from sparkfm_amd import _ffi
    L, h = _ffi.load(), C.c_void_p()
    assert L.fmhip_autoint_model_create(0, shape[0], shape[1], shape[2], lhd[0], lhd[1], lhd[2], None, C.byref(h)) == code
    assert msg.encode() in L.fmhip_last_error() and h.value is None


def small(seed=5, F=3, k=2, L=2, H=2, d=16, n1=12, fields=None):
    rng = np.random.default_rng(seed)
    rows = ref.random_rows(rng, 5, n1, F, [3, 4, 2, 5, 3], one_field_row=False)
    if fields is not None:
        rows = [[(fields[f % len(fields)], i, x) for f, i, x in row] for row in rows]
    layers, u = ref.dense(rng, F, k, L, H, d)
    return ref.State(0.3, rng.normal(0, 0.3, n1), rng.normal(0, 0.3, (n1, k)), layers, u, heads=H), rows, rng.normal(0, 1, 5)


def flat(G):
    return np.concatenate([np.ravel(G["w0"]), G["w"].ravel(), G["v"].ravel()] + [x.ravel() for x in G["layers"]] + [G["u"]])


H_STEP, FD_TOL = 1e-5, 1e-10


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_the_twins_gradient_against_central_differences(loss):
    """F = 3, k = 2, L = 2, H = 2, d = 16, 5 rows; every parameter.  Away from the ReLU's kinks (asserted: no pre-activation within 1e-3 of
    0, so a step of h moves none across) the loss is smooth, the central difference's truncation error falls as h^2 and its rounding error
    grows as 1e-16 / h.  Measured, the worst |difference| / (1 + |g|) under the squared (logistic) loss is 2.42e-7 (7.4e-8) at h = 1e-3,
    2.42e-9 (7.4e-10) at 1e-4, 2.9e-11 (1.3e-11) at 1e-5 — still the h^2 law, and the minimum — then 1.1e-10 (1.3e-10) at 1e-6 and 1.1e-9
    (1.4e-9) at 1e-7, the rounding branch.  h = 1e-5 is used, and the tolerance is 1e-10 (1 + |g|): the h^2 law's 2.4e-11 plus the rounding
    branch's 1e-16 / h = 1e-11, each with a factor 3 (|g| up to 0.52 here).  A wrong term in the chain rule is an
    error of the order of the gradient itself.  Also: a field no row holds is the zero token, and W_0's gradient is exactly 0 on a factor
    slot no row fills (v's column zeroed) — what keeps the device's pad rows of W_0 at 0."""
    s, rows, y = small()
    assert ref.forward(s, rows)["zmin"] > 1e-3
    g = flat(ref.gradients(s, rows, y, loss))

    def value():
        yh = ref.predict(s, rows)[0]
        return float(np.mean(0.5 * (yh - y) ** 2 if loss == "squared" else np.maximum(yh, 0.0) - (y > 0) * yh + np.log1p(np.exp(-np.abs(yh)))))

    arrays = [s.w, s.v] + s.layers + [s.u]
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
    s2, rows2, y2 = small()
    s2.v[:, 1] = 0.0          # factor slot 1 is filled by no row: X_0's column 1 is 0
    G = ref.gradients(s2, rows2, y2, loss)
    assert not G["layers"][0][1].any() and G["layers"][0][0].any() and G["layers"][1].any()


def test_zero_query_and_key_weights_give_the_mean_of_the_values():
    """W_Q = W_K = 0: every score is 0, the attention uniform, so O_f = mean_g V_g for every f and X_1 = relu(mean V + R), to 1e-12."""
    s, rows, _ = small(seed=6, L=1)
    A = s.layers[0].shape[1] // 4
    s.layers[0][:, :2 * A] = 0.0
    o = ref.forward(s, rows)
    X, _, _, V, Ps, Z = o["keep"][0]
    R = X @ s.layers[0][:, 3 * A:]
    assert all(np.abs(P - 1.0 / 3).max() <= 1e-12 for P in Ps)
    assert np.abs(Z - (V.mean(axis=1, keepdims=True) + R)).max() <= 1e-12 and np.abs(o["xl"] - np.maximum(Z, 0)).max() == 0.0
