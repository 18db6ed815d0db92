"""The BPR trainer's redraw mode, host surface (no GPU): the header against the binding and the exported symbols, the refusals that
need no device, the Python keyword, the per-batch fp64 twin (redraw_ref.py) against the per-epoch twins at one batch, and the twins'
held-out NDCG on the harder planted task under both redraws."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import bpr_adaptive_ref as aref
import bpr_ref as bref
import redraw_ref as dref
import train_ref as ref
from train_ref import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDRAW_NAMES = {"fmhip_redraw_" + n for n in ("set", "get", "step", "epoch_stats")}


def declared_in(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))


# ---- symbols -------------------------------------------------------------------------------------------------------------------------

def test_header_matches_the_binding_and_the_library():
    from sparkfm_amd import _build, _ffi
    assert declared_in("fmhip_redraw.h") == set(_ffi.SYMBOLS_REDRAW) == REDRAW_NAMES
    others = (_ffi.SYMBOLS + _ffi.SYMBOLS_EXPERIMENTAL + _ffi.SYMBOLS_TOPK + _ffi.SYMBOLS_PAIRING + _ffi.SYMBOLS_METRICS + _ffi.SYMBOLS_RANKING
              + _ffi.SYMBOLS_WEIGHTS + _ffi.SYMBOLS_RELATIONAL + _ffi.SYMBOLS_MCMC + _ffi.SYMBOLS_MCMC_TASK + _ffi.SYMBOLS_MCMC_GROUPS
              + _ffi.SYMBOLS_MCMC_RELATIONAL + _ffi.SYMBOLS_BPR + _ffi.SYMBOLS_BPR_ADAPTIVE + _ffi.SYMBOLS_WARP + _ffi.SYMBOLS_FTRL)
    assert not REDRAW_NAMES & set(others) and not [n for n in others if n.startswith("fmhip_redraw_")]
    L = _ffi.load()
    for name in _ffi.SYMBOLS_REDRAW:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int, name
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert set(re.findall(r"\bT (fmhip_redraw_[a-z0-9_]+)", out)) == REDRAW_NAMES
    assert os.path.join("..", "..", "include", "fmhip_redraw.h") in _build.HIP_DEPS
    hdr = open(os.path.join(ROOT, "include", "fmhip_redraw.h")).read()
    assert [n for n, _ in _ffi.RedrawStats._fields_] == re.findall(r"int64_t (\w+);", hdr) == ["pairs", "attempts", "forced", "replaced", "violated", "trials"]
    modes = dict(re.findall(r"#define FMHIP_REDRAW_(\w+) (\d+)", hdr))
    assert modes == {"EPOCH": "0", "BATCH": "1"} and (_ffi.REDRAW_EPOCH, _ffi.REDRAW_BATCH) == (0, 1)
    assert _ffi.REDRAWS == {"epoch": 0, "batch": 1}
    # the sampler headers point here and no longer say that there is no per-batch draw
    for name in ("fmhip_bpr_adaptive.h", "fmhip_warp.h"):
        text = open(os.path.join(ROOT, "include", name)).read()
        assert "fmhip_redraw.h" in text and "no per-batch resample" not in text.lower(), name
    # the redraw draws nothing of its own: the sampler's one site
    rng_h = open(os.path.join(ROOT, "sparkfm_amd", "csrc", "mcmc_rng.h")).read()
    assert rng_h.count("t, kStreamNegative);") == 1


def test_c_calls_refuse_null_handles_without_a_device():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    mode = C.c_int(-5)
    st, dr = _ffi.Stats(), _ffi.RedrawStats()
    assert L.fmhip_redraw_set(None, 1) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error()
    assert L.fmhip_redraw_get(None, C.byref(mode)) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error()
    assert mode.value == -5
    assert L.fmhip_redraw_step(None, None, 0, 0, 0.1, 0.0, 0.0, 0.0, C.byref(st), C.byref(dr)) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_redraw_epoch_stats(None, C.byref(dr)) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error()


def small_blocks():
    from sparkfm_amd import DataSet
    users = DataSet.from_rows([(0.0, ([0], [1.0])), (0.0, ([1], [1.0])), (0.0, ([], []))], batch_rows=0)
    items = DataSet.from_rows([(0.0, ([3 + j], [1.0])) for j in range(4)], batch_rows=0)
    return users, items, [[2, 0, 2], [3], []]


def test_python_validates_the_keyword_at_construction():
    from sparkfm_amd import HipBPR
    users, items, pos = small_blocks()
    assert HipBPR.run(users, items, pos).redraw == "epoch"
    assert HipBPR.REDRAWS == ("epoch", "batch")
    for kw in ({}, {"n_candidates": 8}, {"sampler": "warp", "n_candidates": 8}):
        assert HipBPR.run(users, items, pos, redraw="batch", **kw).redraw == "batch"
        assert HipBPR.run(users, items, pos, redraw="epoch", **kw).redraw == "epoch"
    for bad in ("step", "BATCH", "", None, 1, True, ("batch",)):
        with pytest.raises(ValueError, match="redraw must be one of 'epoch', 'batch'"):
            HipBPR.run(users, items, pos, redraw=bad)
    b = HipBPR.run(users, items, pos, redraw="batch")
    with pytest.raises(AttributeError):
        b.redraw = "epoch"                   # fixed at construction
    with pytest.raises(TypeError, match="epoch index"):
        b.step(None, 0, True)                # (want_stats is a keyword: a flag in t's place is refused before any device call)


# ---- the twin ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C_,warp", [(1, False), (4, False), (4, True)])
@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
def test_twin_at_one_batch_equals_the_per_epoch_twins(C_, warp, optimizer):
    """With one batch an epoch's draw and a batch's are the same draw: three epochs of the per-batch twin against bpr_ref /
    bpr_adaptive_ref / warp_ref's, exactly — and with five batches a scored sampler's differ (the uniform one's do not)."""
    P = bref.make_problem(310, 8, n_inter=599, n_neg=2)
    rule = ref.Rule("logistic", True, 1e-10 if optimizer == "adagrad" else None)
    s0 = ref.State(P["w0"], P["w"], P["v"], 0.1 if optimizer == "adagrad" else 0.0)
    run = lambda bp, redraw: dref.epochs(s0.copy(), P, 3, bp, 0.05, 1e-3, 2e-3, 3e-3, rule, C_, warp, 0.1, redraw)      # noqa: E731
    (se, de), (sb, db) = run(0, "epoch"), run(0, "batch")
    assert same((se.w0, se.w, se.v), (sb.w0, sb.w, sb.v)) and np.array_equal(de.neg, db.neg)
    assert np.array_equal(de.weights, db.weights) and np.array_equal(de.trials, db.trials)
    assert np.abs(sb.v - P["v"]).max() > 1e-4
    (se, de), (sb, db) = run(250, "epoch"), run(250, "batch")
    if C_ == 1:
        assert same((se.w0, se.w, se.v), (sb.w0, sb.w, sb.v)) and np.array_equal(de.neg, db.neg)
    else:
        assert not np.array_equal(de.neg, db.neg)
        assert not same((se.w0, se.w, se.v), (sb.w0, sb.w, sb.v))


def test_twin_order_and_range():
    """A batch's draw writes its own pairs alone, and the order given is the order taken."""
    P = bref.make_problem(311, 8, n_inter=599)
    s = ref.State(P["w0"], P["w"], P["v"], 0.0)
    rule = ref.Rule("logistic", True, None)
    D = dref.Draw(P)
    before = D.neg.copy()
    assert np.array_equal(before, bref.draw(P, 0)[0])
    rows = dref.epoch_candidates(P, 5, 4)
    got = dref.batch_step(s, P, D, "best", rows, 256, 512, 1.0, 0.05, 0.0, 0.0, 0.0, rule)
    assert np.array_equal(D.neg[:128], before[:128]) and np.array_equal(D.neg[256:], before[256:])
    assert np.array_equal(D.neg[128:256], got["neg"]) and got["replaced"] > 0
    a, _ = dref.epochs(ref.State(P["w0"], P["w"], P["v"], 0.0), P, 1, 128, 0.05, 0.0, 0.0, 0.0, rule, 4, order=[4, 3, 2, 1, 0])
    b, _ = dref.epochs(ref.State(P["w0"], P["w"], P["v"], 0.0), P, 1, 128, 0.05, 0.0, 0.0, 0.0, rule, 4)
    assert not same((a.w0, a.w, a.v), (b.w0, b.w, b.v))


# ---- the twin's learning ------------------------------------------------------------------------------------------------------------------

# the settings under which test_host_bpr_adaptive.py and test_host_warp.py pin the per-epoch numbers
BEST = dict(k=8, n_neg=3, batch_pairs=128, eta=1.0, regw=1e-3, regv=1e-3, epochs=30, C=8, warp=False, margin=1.0)
WARP = dict(k=8, n_neg=3, batch_pairs=128, eta=0.3, regw=1e-3, regv=1e-3, epochs=30, C=8, warp=True, margin=1.0)


def twin_run(T, S, redraw, seed=3):
    P = aref.task_problem(T, seed, S["k"], S["n_neg"])
    s0 = ref.State(P["w0"], P["w"], P["v"], 0.1)
    s, _ = dref.epochs(s0.copy(), P, S["epochs"], S["batch_pairs"], S["eta"], 0.0, S["regw"], S["regv"], ref.Rule("logistic", True, 1e-10),
                       S["C"], S["warp"], S["margin"], redraw)
    return aref.twin_ndcg(T, P, s)


# the fp64 twin's held-out NDCG@10 on aref.hard_task(3) (2700 pairs in 22 batches of 128), computed here on the CPU
TWIN_NDCG = {("best", "epoch"): 0.3064, ("warp", "epoch"): 0.5554, ("best", "batch"): 0.2712, ("warp", "batch"): 0.5674}


@pytest.mark.parametrize("name,S", [("best", BEST), ("warp", WARP)])
def test_twin_ndcg_on_the_harder_planted_task_under_both_redraws(name, S):
    """The numbers the README and the GPU test quote, from the fp64 twin alone.  Nothing is asserted about which redraw is better."""
    T = aref.hard_task(3)
    assert len(dref.wref.batches(2 * 60 * 15 * S["n_neg"], S["batch_pairs"])) == 22
    got = {redraw: twin_run(T, S, redraw) for redraw in ("epoch", "batch")}
    print("%s: per-epoch %.17g, per-batch %.17g" % (name, got["epoch"], got["batch"]))
    for redraw in ("epoch", "batch"):
        assert got[redraw] == pytest.approx(TWIN_NDCG[(name, redraw)], abs=5e-5), (name, redraw, got[redraw])
