"""The MCMC learner's tasks, host surface (no GPU): the truncated-normal draw of the probit link and its expectation (csrc/mcmc_rng.h
through fmhip_host.cpp, driven by tests/host_probit_harness.cpp — a stand-alone program built with AddressSanitizer and UBSan) against
probit_ref.py's numpy restatement and against the truncated normal's known moments, the new header against the binding, the refusals
that need no device, HipMCMC's validation of `task` and `clip`."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import probit_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = [-3.0, -0.5, 0.0, 0.5, 3.0, 8.0, 40.0]
SEED, N, T = 20261019, 2000, 5            # (the harness draws at t = 5)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("probit") / "host_probit_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "host_probit_harness.cpp"), os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("no sanitizer runtime for g++ in this image")
    assert r.returncode == 0, r.stderr.decode()[-3000:]

    def run(*args):
        r = subprocess.run([exe] + [repr(a) if isinstance(a, float) else str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        return r.stdout.decode()
    return run


@pytest.fixture(scope="module")
def draws(harness):
    """a -> (the library's 2000 draws, their attempt counts), computed once"""
    out = {}
    for a in POINTS:
        rows = [ln.split() for ln in harness("trunc", SEED, a, N).strip().split("\n")]
        out[a] = (from_bits([r[0] for r in rows]), np.array([int(r[1]) for r in rows]))
    return out


def from_bits(words):
    return np.array([int(w, 16) for w in words], np.uint64).view(np.float64)


def ulps(a, b):
    """distance in units of the last place between same-signed doubles"""
    return np.abs(a.view(np.int64) - b.view(np.int64))


def hazard(a):
    """h = phi(a) / Q(a), the mean of z | z > a, from math.erfc; past a = 30 (erfc underflows at a = 37.6) from Mills' ratio's asymptotic
    series Q(a) / phi(a) = (1 - 1/a^2 + 3/a^4 - 15/a^6 + 105/a^8 - ...) / a, whose next term is below 2e-12 there"""
    if a > 30.0:
        return a / (1.0 - a ** -2 + 3.0 * a ** -4 - 15.0 * a ** -6 + 105.0 * a ** -8)
    return math.exp(-0.5 * a * a) / math.sqrt(2.0 * math.pi) / (0.5 * math.erfc(a / math.sqrt(2.0)))


# ---- the draw: library against reference ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("a", POINTS)
def test_truncated_normal_of_the_library_is_the_references(draws, a):
    """2000 draws a truncation point: the same number of attempts, the values to 4 ulp (libm and numpy may differ in the last bits of
    log / cos / exp), every one above its truncation point."""
    lib, attempts = draws[a]
    ref, ref_attempts, margin = PR.truncated_normal(SEED, np.arange(N), T, np.full(N, a))
    assert len(lib) == N and np.array_equal(attempts, ref_attempts), (attempts.max(), ref_attempts.max())
    assert (np.sign(lib) == np.sign(ref)).all() and ulps(lib, ref).max() <= 4, ulps(lib, ref).max()
    assert (lib > a).all() and (ref > a).all()
    assert margin > 0.0 and len(np.unique(lib)) == N
    if a in (-0.5, 0.0, 0.5, 3.0):
        assert attempts.max() > 1           # the rejection path was taken
    assert attempts.max() < 64


@pytest.mark.parametrize("a", POINTS)
def test_moments_of_the_truncated_normal(draws, a):
    """The 2000 draws: the mean within 5 standard errors of h = phi(a) / Q(a), the variance within 5 standard errors of 1 + a h - h^2;
    the sample variance's own variance is (mu_4 - sigma^4) / n with the central fourth moment mu_4 taken from 200,000 draws of the
    reference (another seed)."""
    z = draws[a][0]
    h = hazard(a)
    var = 1.0 + a * h - h * h
    big = PR.truncated_normal(77, np.arange(200000), T, np.full(200000, a))[0]
    mu4 = float(np.mean((big - big.mean()) ** 4))
    assert abs(big.mean() - h) <= 5.0 * math.sqrt(var / len(big)) and abs(big.var() - var) <= 5.0 * math.sqrt((mu4 - var ** 2) / len(big))
    assert abs(z.mean() - h) <= 5.0 * math.sqrt(var / N), (z.mean(), h)
    assert abs(z.var() - var) <= 5.0 * math.sqrt((mu4 - var ** 2) / N), (z.var(), var)


def test_the_last_attempt_is_taken_unconditionally():
    """The reference's own bound (the library's is exercised by the harness): no draw takes more than 64 attempts, whatever a holds."""
    for a in (np.nan, np.inf, 1e300):
        z, attempts, _ = PR.truncated_normal(3, np.arange(5), 1, np.full(5, a))
        assert (attempts == 64).all()
    z, attempts, _ = PR.truncated_normal(3, np.arange(5), 1, np.full(5, -np.inf))
    assert (attempts == 1).all() and np.isfinite(z).all()


# ---- the expectation -----------------------------------------------------------------------------------------------------------

def test_expectation_without_sampling(harness):
    """E[z | z > a] on a grid up to a = 1000: finite, at least max(a, 0), the reference's to 1e-12 relative; continuous across a = 30,
    where the asymptote takes over, to 1e-3 relative."""
    grid = np.concatenate([np.linspace(-1000.0, -40.0, 25), np.linspace(-38.0, 38.0, 153), np.linspace(40.0, 1000.0, 25), [29.999999, 30.0, 30.000001]])
    lib = from_bits(harness("mean", *[float(a) for a in grid]).split())
    assert len(lib) == len(grid) and np.isfinite(lib).all()
    assert (lib >= np.maximum(grid, 0.0)).all()
    np.testing.assert_allclose(lib, PR.truncated_mean(grid), rtol=1e-12, atol=1e-290)
    below, at, above = lib[-3:]
    assert abs(above - at) <= 1e-3 * at and abs(below - at) <= 1e-3 * at
    for a in (-3.0, 0.0, 0.5, 8.0, 29.0):
        assert lib[np.argmin(np.abs(grid - a))] == pytest.approx(hazard(float(grid[np.argmin(np.abs(grid - a))])), rel=1e-12)


def test_host_arithmetic_under_the_sanitizers(harness):
    """Draws over truncation points from -1e300 to 1e300, ones that are not finite, the expectation's range, the task validation."""
    for seed in (20261019, 5):
        assert "checks ok" in harness("check", seed)


# ---- symbols -------------------------------------------------------------------------------------------------------------

def test_header_matches_the_binding():
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_mcmc_task.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fmhip_mcmc_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_ffi.SYMBOLS_MCMC_TASK) == {"fmhip_mcmc_task_opts_default", "fmhip_mcmc_create_task", "fmhip_mcmc_latent_targets"}
    others = (_ffi.SYMBOLS + _ffi.SYMBOLS_EXPERIMENTAL + _ffi.SYMBOLS_TOPK + _ffi.SYMBOLS_PAIRING + _ffi.SYMBOLS_METRICS + _ffi.SYMBOLS_RANKING
              + _ffi.SYMBOLS_WEIGHTS + _ffi.SYMBOLS_RELATIONAL + _ffi.SYMBOLS_MCMC)
    assert not set(_ffi.SYMBOLS_MCMC_TASK) & set(others)
    assert '#include "fmhip_mcmc.h"' in code
    L = _ffi.load()
    for name in _ffi.SYMBOLS_MCMC_TASK:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert any(d.endswith("fmhip_mcmc_task.h") for d in _build.HIP_DEPS)
    fields = re.search(r"typedef struct \{(.*?)\} fmhip_mcmc_task_opts;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)\s*[,;]", fields) == [n for n, _ in _ffi.McmcTaskOpts._fields_]
    assert int(re.search(r"#define FMHIP_MCMC_REGRESSION (\d+)", code).group(1)) == _ffi.MCMC_REGRESSION == 0
    assert int(re.search(r"#define FMHIP_MCMC_CLASSIFICATION (\d+)", code).group(1)) == _ffi.MCMC_CLASSIFICATION == 1
    o = _ffi.McmcTaskOpts(9, 9, 9.0, 9.0)
    assert L.fmhip_mcmc_task_opts_default(C.byref(o)) == 0 and (o.task, o.clip, o.clip_lo, o.clip_hi) == (0, 0, 0.0, 0.0)
    # fmhip_mcmc.h says where the tasks went
    old = open(os.path.join(ROOT, "include", "fmhip_mcmc.h")).read()
    assert "fmhip_mcmc_task.h" in old and "task" not in re.sub(r"/\*.*?\*/", "", old, flags=re.S)


# ---- refusals that need no device ----------------------------------------------------------------------------------------------

def test_c_calls_refuse_bad_tasks_and_null_handles_without_a_device():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    h = C.c_void_p(7)
    nan, inf = float("nan"), float("inf")
    assert L.fmhip_mcmc_task_opts_default(None) == -1 and b"task_opts is NULL" in L.fmhip_last_error()
    for task, words in ((_ffi.McmcTaskOpts(2, 0, 0.0, 0.0), b"unknown task"), (_ffi.McmcTaskOpts(-1, 0, 0.0, 0.0), b"unknown task"),
                        (_ffi.McmcTaskOpts(1, 1, 1.0, 5.0), b"clip goes with the regression task"), (_ffi.McmcTaskOpts(0, 1, 5.0, 1.0), b"clip range"),
                        (_ffi.McmcTaskOpts(0, 1, 2.0, 2.0), b"clip range"), (_ffi.McmcTaskOpts(0, 1, nan, 1.0), b"clip range"),
                        (_ffi.McmcTaskOpts(0, 1, 0.0, inf), b"clip range")):
        h.value = 7
        assert L.fmhip_mcmc_create_task(None, None, None, None, C.byref(task), C.byref(h)) == -1 and h.value is None
        assert words in L.fmhip_last_error(), L.fmhip_last_error()
    # what fmhip_mcmc_create refuses, in the same words
    assert L.fmhip_mcmc_create_task(None, None, None, None, None, None) == -1 and b"out is NULL" in L.fmhip_last_error()
    for task in (None, _ffi.McmcTaskOpts(1, 0, 0.0, 0.0), _ffi.McmcTaskOpts(0, 1, 1.0, 5.0)):
        ref = None if task is None else C.byref(task)
        assert L.fmhip_mcmc_create_task(None, None, None, None, ref, C.byref(h)) == -1 and b"model or train set is NULL" in L.fmhip_last_error()
        o = _ffi.McmcOpts()
        L.fmhip_mcmc_opts_default(C.byref(o))
        o.gamma_0 = 0.0
        assert L.fmhip_mcmc_create(None, None, None, C.byref(o), C.byref(h)) == -1
        words = L.fmhip_last_error()
        assert L.fmhip_mcmc_create_task(None, None, None, C.byref(o), ref, C.byref(h)) == -1 and L.fmhip_last_error() == words and b"gamma_0" in words
    out = np.zeros(4)
    assert L.fmhip_mcmc_latent_targets(None, _ffi.ptr(out)) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_mcmc_latent_targets(h, None) == -1 and b"NULL" in L.fmhip_last_error()


def test_hipmcmc_validates_task_and_clip():
    from sparkfm_amd import HipMCMC
    m = HipMCMC.run()
    assert (m.task, m.clip) == ("regression", None)
    m = HipMCMC.run(task="classification", seed=3)
    assert (m.task, m.clip, m.seed) == ("classification", None, 3)
    assert HipMCMC.run(clip=(1, 5)).clip == (1.0, 5.0) and HipMCMC.run(clip="labels").clip == "labels" and HipMCMC.run(clip=[0.5, 0.75]).clip == (0.5, 0.75)
    for kw in (dict(task="ranking"), dict(task=1), dict(task=None), dict(task="classification", clip=(0, 1)), dict(task="classification", clip="labels"),
               dict(clip=(5, 1)), dict(clip=(1, 1)), dict(clip=(float("nan"), 1)), dict(clip=(0, float("inf"))), dict(clip="range"), dict(clip=(1, 2, 3)),
               dict(clip=3.0), dict(clip=("a", "b"))):
        with pytest.raises(ValueError):
            HipMCMC.run(**kw)
    # no handle before the first learn
    with pytest.raises(RuntimeError, match="first learn"):
        HipMCMC.run(task="classification").latent_targets()
    # the scores belong to their task, whether or not a handle exists yet
    with pytest.raises(ValueError, match="computeLogLoss"):
        HipMCMC.run(task="classification").computeRMSE()
    for name in ("computeLogLoss", "computeAccuracy", "computeAUC"):
        with pytest.raises(ValueError, match="classification"):
            getattr(HipMCMC.run(), name)()
