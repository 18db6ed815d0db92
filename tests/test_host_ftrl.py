"""FTRL-Proximal without a GPU: the header against the binding and the exported symbols, the C ABI's argument checks, the Python
learners' keyword validation, and the tests' own twin (ftrl_ref.py) — pinned to AdaGrad where the two rules coincide, at its exact
cases (g == 0, the L1 threshold, an underflowing g^2), and its fp32 form against its fp64 form on the GPU tests' one-step problems:
rounding alone must keep the zero pattern inside the cap those tests allow the device."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import ftrl_ref as fref
from train_ref import adagrad_rule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FTRL_NAMES = {"fmhip_model_set_ftrl", "fmhip_model_get_ftrl_state", "fmhip_model_set_ftrl_state", "fmhip_model_nonzeros"}


def L():
    from sparkfm_amd import _ffi
    return _ffi.load()


def declared_in(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))


# ---- symbols ------------------------------------------------------------------------------------------------------------

def test_header_matches_the_binding_and_the_library():
    from sparkfm_amd import _build, _ffi
    assert declared_in("fmhip_ftrl.h") == set(_ffi.SYMBOLS_FTRL) == FTRL_NAMES
    others = (_ffi.SYMBOLS + _ffi.SYMBOLS_EXPERIMENTAL + _ffi.SYMBOLS_TOPK + _ffi.SYMBOLS_PAIRING + _ffi.SYMBOLS_METRICS + _ffi.SYMBOLS_RANKING
              + _ffi.SYMBOLS_WEIGHTS + _ffi.SYMBOLS_RELATIONAL + _ffi.SYMBOLS_MCMC + _ffi.SYMBOLS_MCMC_TASK + _ffi.SYMBOLS_MCMC_GROUPS
              + _ffi.SYMBOLS_MCMC_RELATIONAL + _ffi.SYMBOLS_BPR + _ffi.SYMBOLS_BPR_ADAPTIVE + _ffi.SYMBOLS_WARP)
    assert not FTRL_NAMES & set(others)
    lib = L()
    for name in _ffi.SYMBOLS_FTRL:
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int, name
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert set(re.findall(r"\bT (fmhip_[a-z0-9_]*ftrl[a-z0-9_]*)", out)) == FTRL_NAMES - {"fmhip_model_nonzeros"}
    assert "fmhip_model_nonzeros" in re.findall(r"\bT (fmhip_[a-z0-9_]+)", out)
    assert os.path.join("..", "..", "include", "fmhip_ftrl.h") in _build.HIP_DEPS
    hdr = open(os.path.join(ROOT, "include", "fmhip_ftrl.h")).read()
    assert re.search(r"FMHIP_OPT_FTRL\s*=\s*2\b", hdr) and _ffi.OPT_FTRL == 2
    # FTRL is no third value of optimizer=: the names and the setter of the other two rules are what they were
    assert _ffi.OPTIMIZERS == {"sgd": 0, "adagrad": 1}
    assert "fmhip_model_set_ftrl" not in declared_in("fmhip.h")


def test_set_optimizer_still_refuses_2_and_names_the_ftrl_setter():
    assert L().fmhip_model_set_optimizer(None, 2, 1e-10, 0.1) == -1
    msg = L().fmhip_last_error().decode()
    assert "optimizer" in msg and "fmhip_model_set_ftrl" in msg, msg


# ---- the C ABI's argument checks (before the model is looked at: a NULL model gets the same answer) -----------------------

@pytest.mark.parametrize("args,names", [((-1.0, 0.1, 0.0, 0.0), "beta"), ((math.nan, 0.1, 0.0, 0.0), "beta"), ((math.inf, 0.1, 0.0, 0.0), "beta"),
                                        ((1.0, -0.1, 0.0, 0.0), "initial_accumulator"), ((1.0, math.nan, 0.0, 0.0), "initial_accumulator"),
                                        ((1.0, math.inf, 0.0, 0.0), "initial_accumulator"),
                                        ((1.0, 0.1, -1e-9, 0.0), "l1w"), ((1.0, 0.1, math.inf, 0.0), "l1w"), ((1.0, 0.1, math.nan, 0.0), "l1w"),
                                        ((1.0, 0.1, 0.0, -2.0), "l1v"), ((1.0, 0.1, 0.0, math.nan), "l1v"), ((1.0, 0.1, 0.0, math.inf), "l1v"),
                                        ((0.0, 0.0, 0.0, 0.0), "beta + sqrt(initial_accumulator)"),
                                        ((1e-60, 0.0, 0.0, 0.0), "beta + sqrt(initial_accumulator)")])
def test_set_ftrl_refuses_bad_settings(args, names):
    assert L().fmhip_model_set_ftrl(None, *args) == -1
    msg = L().fmhip_last_error().decode()
    assert names in msg and "NULL" not in msg, msg


def test_ftrl_calls_refuse_a_null_model():
    lib = L()
    assert lib.fmhip_model_set_ftrl(None, 1.0, 0.0, 0.0, 0.0) == -1 and b"NULL" in lib.fmhip_last_error()
    assert lib.fmhip_model_set_ftrl(None, 0.0, 0.1, 1.0, 1.0) == -1 and b"NULL" in lib.fmhip_last_error()
    z0, n0 = C.c_double(), C.c_double()
    buf = np.zeros(4)
    p = buf.ctypes.data_as(C.c_void_p)
    assert lib.fmhip_model_get_ftrl_state(None, C.byref(z0), p, p, C.byref(n0), p, p) == -1 and b"NULL" in lib.fmhip_last_error()
    assert lib.fmhip_model_set_ftrl_state(None, 0.0, p, p, 0.0, p, p) == -1 and b"NULL" in lib.fmhip_last_error()
    assert lib.fmhip_model_set_ftrl_state(None, math.nan, p, p, 0.0, p, p) == -1 and b"z0" in lib.fmhip_last_error()
    assert lib.fmhip_model_set_ftrl_state(None, 0.0, p, p, -1.0, p, p) == -1 and b"n0" in lib.fmhip_last_error()
    assert lib.fmhip_model_set_ftrl_state(None, 0.0, p, p, math.inf, p, p) == -1 and b"n0" in lib.fmhip_last_error()
    w = C.c_int64()
    assert lib.fmhip_model_nonzeros(None, C.byref(w), None, None) == -1 and b"NULL" in lib.fmhip_last_error()
    # the AdaGrad state calls are what they were
    assert lib.fmhip_model_get_optimizer_state(None, C.byref(n0), p, p) == -1


# ---- the learners' keywords ----------------------------------------------------------------------------------------------

BAD_KW = [dict(alpha=-0.1), dict(alpha=math.nan), dict(beta=-1.0), dict(beta=math.inf), dict(l1w=-1.0), dict(l1w=math.nan), dict(l1v=-0.5),
          dict(l1v=math.inf), dict(l2_0=-1.0), dict(l2w=-1e-3), dict(l2v=math.nan), dict(ftrl_init=-0.1), dict(ftrl_init=math.nan),
          dict(beta=0.0, ftrl_init=0.0), dict(loss="hinge"), dict(pairs=1)]


@pytest.mark.parametrize("kw", BAD_KW)
def test_learners_validate_their_keywords(kw):
    from sparkfm_amd import HipDataParallelFTRL, HipFTRL
    with pytest.raises(ValueError):
        HipFTRL.run(**kw)
    with pytest.raises(ValueError):
        HipDataParallelFTRL(None, **kw)          # (validated before the communicator is touched)


def test_learner_keywords_and_defaults():
    import inspect
    import sparkfm_amd
    from sparkfm_amd import HipFTRL, HipSGD, _ffi
    from sparkfm_amd.distributed import HipDataParallelFTRL, HipDataParallelSGD
    assert sparkfm_amd.HipFTRL is HipFTRL and sparkfm_amd.HipDataParallelFTRL is HipDataParallelFTRL
    assert issubclass(HipFTRL, HipSGD) and issubclass(HipDataParallelFTRL, HipDataParallelSGD)
    sig = inspect.signature(HipFTRL.__init__)
    want = dict(alpha=0.1, beta=1.0, l1w=0.0, l1v=0.0, l2_0=0.0, l2w=0.0, l2v=0.0, ftrl_init=0.0, loss="squared", pairs=False, shuffle_seed=None)
    assert {n: p.default for n, p in sig.parameters.items() if n != "self"} == want
    dp = inspect.signature(HipDataParallelFTRL.__init__).parameters
    assert all(dp[n].default == v for n, v in want.items() if n != "shuffle_seed")
    f = HipFTRL.run(alpha=0.2, beta=0.5, l1w=1.0, l1v=0.25, l2_0=1e-3, l2w=2e-3, l2v=3e-3, ftrl_init=0.1, loss="logistic", pairs=True, shuffle_seed=4)
    assert (f.eta, f.reg0, f.regw, f.regv) == (0.2, 1e-3, 2e-3, 3e-3) and (f.alpha, f.l2_0, f.l2w, f.l2v) == (0.2, 1e-3, 2e-3, 3e-3)
    assert (f.beta, f.ftrl_init, f.l1w, f.l1v, f.loss, f.pairs, f.shuffle_seed) == (0.5, 0.1, 1.0, 0.25, "logistic", True, 4)
    assert isinstance(f.rule, _ffi.FtrlRule) and isinstance(f.rule, _ffi.TrainRule) and f.rule.opt_code == _ffi.OPT_FTRL
    assert (f.rule.loss_code, f.rule.pairing_code) == (_ffi.LOSS_LOGISTIC, _ffi.PAIRING_ADJACENT)
    with pytest.raises(ValueError):
        f.rule.require_default()
    with pytest.raises(TypeError):
        HipFTRL.run(optimizer="ftrl")             # no third value of optimizer=, here either
    with pytest.raises(TypeError):
        HipFTRL.run(eta=0.1)


# ---- the twin -------------------------------------------------------------------------------------------------------------

def test_twin_without_l1_l2_is_adagrad_with_eps_beta():
    """l1 = l2 = 0, beta = eps: theta' = theta - eta*g / (beta + sqrt(n')) — 20 steps of a changing gradient (and a changing eta:
    no state depends on it), 1e-12."""
    rng = np.random.default_rng(5)
    eps, init = 1e-3, 0.1
    theta = rng.normal(0, 0.3, 500)
    ta, na = theta.copy(), np.full(500, init)
    tf, nf, zf = theta.copy(), np.full(500, init), fref.zeta_init(theta, np.full(500, init), eps)
    for i in range(20):
        g = rng.normal(0, 1.0, 500) * rng.choice([1e-3, 1.0, 30.0], 500)
        eta = 0.05 * (1 + i % 3)
        ta, na = adagrad_rule(ta, na, g, eta, eps)
        tf, zf, nf = fref.ftrl_rule(tf, zf, nf, g, eta, 0.0, 0.0, eps)
        assert np.abs(tf - ta).max() <= 1e-12 * max(1.0, np.abs(ta).max()) and np.array_equal(nf, na)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_twin_exact_cases(dtype):
    t = dtype
    theta, zeta, n = np.array([0.3, -0.2, 0.0, 1.5], t), np.array([-0.4, 0.1, 0.0, -7.0], t), np.array([0.0, 0.5, 0.0, 2.0], t)
    # g == 0 moves nothing — even at n = 0, even where the closed form would give another theta, under any l1 / l2
    for l1, l2 in ((0.0, 0.0), (3.0, 0.5)):
        t1, z1, n1 = fref.ftrl_rule(theta, zeta, n, np.zeros(4, t), 0.1, l1, l2, 0.5, t)
        assert t1.dtype == t and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in ((t1, theta), (z1, zeta), (n1, n)))
    t1, _, _ = fref.ftrl_rule(theta, zeta, n, np.array([-0.0, 0.0, -0.0, 0.0], t), 0.1, 0.0, 0.0, 0.5, t)
    assert np.array_equal(t1, theta)
    # |zeta'| <= tau gives exactly +0 (the threshold itself included)
    g = np.array([1.0, -1.0, 0.5, 2.0], t)
    _, z1, _ = fref.ftrl_rule(theta, zeta, n, g, 0.1, 0.0, 0.0, 0.5, t)
    l1 = float(np.abs(z1[0])) / 0.1
    while t(t(0.1) * t(l1)) < np.abs(z1[0]):
        l1 = np.nextafter(t(l1), t(np.inf))
    t1, z1b, _ = fref.ftrl_rule(theta, zeta, n, g, 0.1, l1, 0.0, 0.5, t)
    assert np.array_equal(z1, z1b)
    zero = np.abs(z1) <= t(t(0.1) * t(l1))
    assert zero[0] and not zero.all()
    assert (t1[zero] == 0).all() and not np.signbit(t1[zero]).any() and (t1[~zero] != 0).all()
    assert (np.sign(t1[~zero]) == -np.sign(z1[~zero])).all()
    # g = 1e-30 at n = 0: g^2 underflows (fp32), r + r0 = 0 — the guard, no NaN; theta follows zeta' = zeta + eta*g
    t1, z1, n1 = fref.ftrl_rule(np.zeros(2, t), np.zeros(2, t), np.zeros(2, t), np.array([1e-30, -1e-30], t), 0.1, 0.0, 0.0, 0.5, t)
    assert np.isfinite(t1).all() and np.isfinite(z1).all() and np.isfinite(n1).all()
    assert (z1 != 0).all() and (np.sign(t1) == -np.sign(z1)).all()
    if t is np.float32:
        assert (n1 == 0).all()


def test_state_is_the_proximal_centre():
    """zeta = -theta (beta + sqrt(n)): with l1 = l2 = 0 the closed form returns theta, so an initialised V survives."""
    rng = np.random.default_rng(2)
    s = fref.State(0.3, rng.normal(0, 0.1, 7), rng.normal(0, 0.05, (3, 7)), init=0.25, beta=0.5)
    assert np.allclose(-s.zv / (0.5 + np.sqrt(s.nv)), s.v, rtol=1e-15, atol=0) and s.z0 == -0.3 * (0.5 + 0.5)
    c = s.copy()
    c.v[0, 0] = 9.0
    assert s.v[0, 0] != 9.0


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k", fref.KS)
@pytest.mark.parametrize("path", ["dense", "rows"])
def test_fp32_twin_keeps_the_zero_pattern_inside_the_cap(k, loss, path):
    """The GPU tests' one-step problems in the twin's fp32 form against its fp64 form: 30-70 % of the touched coordinates land on
    zero under the L1 the twin chooses, the two zero patterns differ only at coordinates within the tolerance of the threshold, and
    those number at most 1 % of the touched ones — the condition test_gpu_ftrl.py puts to the device."""
    a = fref.one_step_problem(k, loss, path)
    l1w, l1v = fref.choose_l1(a, loss)
    rule = fref.Rule(loss, False, fref.BETA, l1w, l1v)
    args = (a["row_ptr"], a["col"], a["val"], a["y"], 0, len(a["y"]), fref.ETA) + fref.L2 + (rule,)
    s0 = fref.State(a["w0"], a["w"], a["v"], fref.INIT, fref.BETA)
    s1 = fref.step(s0.copy(), *args)
    f0 = fref.State(a["w0"], a["w"], a["v"], fref.INIT, fref.BETA, np.float32)
    f1 = fref.step(f0.copy(), *args)
    near = fref.near_threshold(s0, s1, fref.ETA, rule)
    assert all(np.array_equal(g64 != 0, g32 != 0) for g64, g32 in zip(s1.g[1:], f1.g[1:]))
    for name, touched in (("w", s1.g[1] != 0), ("v", s1.g[2] != 0)):
        zero64, zero32 = (getattr(s1, name) == 0) & touched, (getattr(f1, name) == 0) & touched
        share = zero64.sum() / touched.sum()
        assert 0.3 <= share <= 0.7, (name, share)
        assert not ((zero64 != zero32) & ~near[name]).any(), name
        assert near[name].sum() <= fref.ZERO_CAP * touched.sum(), (name, int(near[name].sum()), int(touched.sum()))
        # untouched coordinates keep their bits
        assert np.array_equal(getattr(f1, name)[~touched], getattr(f0, name)[~touched])
    tol = fref.tolerances(s0, s1)
    for name in ("v", "w", "zv", "zw", "nv", "nw"):
        d64 = getattr(s1, name) - getattr(s0, name)
        d32 = getattr(f1, name).astype(np.float64) - getattr(f0, name).astype(np.float64)
        far = ~near[name[-1]]
        assert (np.abs(d32 - d64)[far] <= tol[name][far]).all(), name
