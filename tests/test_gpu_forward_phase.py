"""The forward's issue-priority instances (fmhip_tune key FORWARD_KERNEL = 60, the default: the w-tile kernel;
include/fmhip_experimental.h) against the plain walk of the same kernel (61): scheduling only.  The priority changes WHEN a
wave issues its loads, never the order of a row's sums, so every bit of the residuals, the q terms, the predictions, the
parameters after three SGD steps with weight decay and that step's statistics must be those of the plain walk — two models
over one dataset in one process, the key set per model (fmhip_model_tune).  The bit test alone would pass if both were wrong
together: at the default key the residuals are also checked against the oracle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
from sparkfm_amd import _ffi

pytestmark = pytest.mark.gpu

TOL_Y = 1e-5        # tests/test_gpu_parity.py, TOL_Y: |d| <= 1e-5 * (1 + sum|terms|) for yhat and e
ROWS, FEATS, BATCH = 2998, 600, 1500      # batches of 1500 and 1498 rows: more than one (the dense hot block exists), even (pairs), no multiple of 8
HOT = 20            # the first ids: each in > 10 % of the rows
EDGE_LENGTHS = (0, 1, 7, 8, 9, 16, 17, 63, 64, 65)     # around the 8-entry step and its multiples


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def make_problem(seed=5300):
    """CSR rows of the edge lengths (six times over) and then U{1..70}; ids distinct within a row, the first HOT ids drawn
    with probability 0.3 each (so that they pass the hot block's 10 % density test), the rest uniform over the cold ids."""
    rng = np.random.default_rng(seed)
    lengths = np.concatenate([np.tile(EDGE_LENGTHS, 6), rng.integers(1, 71, ROWS - 6 * len(EDGE_LENGTHS))])
    col, val = [], []
    for n in lengths:
        hot = np.flatnonzero(rng.random(HOT) < 0.3)[:n]
        cold = HOT + rng.choice(FEATS - HOT, size=n - len(hot), replace=False)
        idx = np.concatenate([hot, cold]).astype(np.int32)
        rng.shuffle(idx)
        col.append(idx)
        val.append(np.where(rng.random(n) < 0.5, 1.0, rng.uniform(0.1, 1.0, n)))
    row_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    col = np.concatenate(col).astype(np.int32)
    col[row_ptr[-2]] = FEATS - 1              # the last id occurs: dimension == FEATS - 1
    y = rng.normal(0, 1.0, ROWS)
    return dict(n1=FEATS, row_ptr=row_ptr, col=col, val=np.concatenate(val), y=y, y01=(rng.random(ROWS) < 0.4).astype(np.float64),
                weights=rng.uniform(0.25, 2.0, ROWS), seed=seed)


@pytest.fixture(scope="module")
def problem():
    return make_problem()


def params(a, k):
    rng = np.random.default_rng(a["seed"] + k)
    return float(rng.normal(0, 0.1)), rng.normal(0, 0.1, a["n1"]), rng.normal(0, 0.1, (k, a["n1"]))


# name -> k, flat addresses, loss, pairs, weighted
CASES = {
    "k32": dict(k=32),                                   # unpacked rows, w tile
    "k16-packed": dict(k=16),                            # packed rows, plain kernel
    "k64": dict(k=64),                                   # two float4 per lane
    "k32-flat": dict(k=32, flat=True),                   # 64-bit addresses: the walk without look-ahead
    "k32-logistic": dict(k=32, loss="logistic"),
    "k32-paired": dict(k=32, loss="logistic", pairs=True),   # q-mode forward
    "k32-weighted": dict(k=32, weighted=True),               # q-mode forward
}


def outputs(fmhip, ds, a, case, key):
    """everything the forward feeds, as raw bytes-comparable arrays, for one model with FORWARD_KERNEL = key"""
    L = _ffi.load()
    k = case["k"]
    fm = fmhip.FMModel(a["n1"] - 1, k)
    fm.w0, fm.w, fm.v = params(a, k)
    h = fm.handle
    _ffi.check(L.fmhip_model_tune(h, _ffi.TUNE_FORWARD_KERNEL, key))
    if case.get("flat"):
        _ffi.check(L.fmhip_model_tune(h, _ffi.TUNE_FLAT_ADDRESS, 1))
    if case.get("loss"):
        _ffi.check(L.fmhip_model_set_loss(h, _ffi.loss_code(case["loss"])))
    if case.get("pairs"):
        _ffi.check(L.fmhip_model_set_pairing(h, _ffi.pairing_code(True)))
    out = {"residual": fm.residual(ds), "term_q": fm.termQ(ds), "predict": fm.predict(ds)}
    for j in range(3):
        _ffi.check(L.fmhip_sgd_step(h, ds.handle, j % ds.n_batches, 0.02, 0.0, 1e-3, 1e-3, None))
    st = _ffi.Stats()
    _ffi.check(L.fmhip_step_stats(h, C.byref(st)))
    fm._device_updated()
    w, v = fm.rows(np.arange(a["n1"], dtype=np.int32))
    out.update(w=w, v=v, w0=np.float64(fm.w0), stats=np.array([st.sse, st.sum_e, st.rows, st.nnz, st.nonfinite, st.steps], np.float64))
    fm.close(discard=True)
    return out


def dataset(fmhip, a, case):
    y = a["y01"] if case.get("loss") == "logistic" else a["y"]
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], y, batch_rows=BATCH, weights=a["weights"] if case.get("weighted") else None).cache()
    assert ds.n_batches == 2 and len(ds.layout()["hot_ids"]) > 0, ds.layout()       # the dense hot block's prologue runs
    return ds


# (value with the raised issue priority, the same kernel without it): the w-tile kernel, the only one that raises it; the plain
# kernel's pair of values must agree too (it ignores the bit)
VARIANTS = [(_ffi.FWD_WTILE, _ffi.FWD_WTILE | _ffi.FWD_NO_ISSUE_PRIO), (_ffi.FWD_PLAIN, _ffi.FWD_PLAIN | _ffi.FWD_NO_ISSUE_PRIO)]


@pytest.mark.parametrize("name", list(CASES))
def test_every_variant_gives_the_plain_walk_s_bits(fmhip, problem, name):
    case = CASES[name]
    ds = dataset(fmhip, problem, case)
    for key, plain in VARIANTS:
        want = outputs(fmhip, ds, problem, case, plain)
        assert want["stats"][4] == 0 and np.isfinite(want["v"]).all()
        got = outputs(fmhip, ds, problem, case, key)
        for what in want:
            p, q = np.ascontiguousarray(got[what]), np.ascontiguousarray(want[what])
            assert p.shape == q.shape and p.dtype == q.dtype and p.tobytes() == q.tobytes(), (name, key, what)
    ds.unpersist()


def term_scale(a, w0, w, v):
    """1 + sum of |terms| of the forward per row (the yhat tolerance's scale, as tests/test_gpu_parity.py forms it)"""
    out = np.ones(len(a["y"]))
    for r in range(len(a["y"])):
        s = slice(a["row_ptr"][r], a["row_ptr"][r + 1])
        idx, x = a["col"][s], a["val"][s]
        t = np.abs(v[:, idx] * x)
        out[r] += abs(w0) + np.abs(w[idx] * x).sum() + 0.5 * ((t.sum(axis=1) ** 2).sum() + (t * t).sum())
    return out


@pytest.mark.parametrize("name", ["k32", "k16-packed"])
def test_default_variant_against_the_oracle(fmhip, problem, name):
    a, case = problem, CASES[name]
    ds = dataset(fmhip, a, case)
    w0, w, v = params(a, case["k"])
    fm = fmhip.FMModel(a["n1"] - 1, case["k"])
    fm.w0, fm.w, fm.v = w0, w, v
    _ffi.check(_ffi.load().fmhip_model_tune(fm.handle, _ffi.TUNE_FORWARD_KERNEL, _ffi.FWD_DEFAULT))
    e = fm.residual(ds)
    oe = oracle.residual(w0, w, v, a["row_ptr"], a["col"], a["val"], a["y"])
    sc = term_scale(a, w0, w, v)
    assert (np.abs(e - oe) <= TOL_Y * sc).all(), float((np.abs(e - oe) / sc).max())
    fm.close(discard=True)
    ds.unpersist()


def test_default_key_is_what_the_design_says(fmhip):
    """DESIGN.md section 4 names the shipped default of the forward-kernel key: the library starts with it, it has the issue
    priority on (bit 0 clear), and the library carries no timing-only ablation."""
    L = _ffi.load()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = re.search(r"`FMHIP_TUNE_FORWARD_KERNEL` defaults to (\d+)", open(os.path.join(root, "DESIGN.md")).read())
    assert m and int(m.group(1)) == _ffi.FWD_DEFAULT and not _ffi.FWD_DEFAULT & _ffi.FWD_NO_ISSUE_PRIO
    # the defaults the library starts with: g_tune's initialiser, one value per key in the enum's order
    src = open(os.path.join(root, "sparkfm_amd", "csrc", "fm_forward.hip")).read()
    init = [int(x) for x in re.search(r"g_tune\[kTuneCount\] = \{([^}]*)\}", src).group(1).split(",")]
    assert len(init) == len(_ffi.TUNE) and init[_ffi.TUNE_FORWARD_KERNEL] == _ffi.FWD_DEFAULT
    assert L.fmhip_ablation_mask() == 0
