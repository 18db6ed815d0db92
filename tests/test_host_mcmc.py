"""The MCMC learner, host surface (no GPU): the counter-based generator of the library (csrc/mcmc_rng.h through fmhip_host.cpp, driven by
tests/host_mcmc_harness.cpp — a stand-alone program built with AddressSanitizer and UBSan) against the published known answers and
against mcmc_ref.py's independent numpy implementation, the moments of its normal and gamma, the header against the binding, the
refusals that need no device, HipMCMC's argument validation."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mcmc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = ["6627e8d5 e169c58d bc57ac4c 9b00dbd8", "408f276d 41c83b0e a20bc7c6 6d5451fd", "d16cfe09 94fdcceb 5001e420 24126ea1"]
KAT_INPUTS = [((0, 0, 0, 0), (0, 0)), ((0xffffffff,) * 4, (0xffffffff,) * 2),
              ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mcmc") / "host_mcmc_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "host_mcmc_harness.cpp"), os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("no sanitizer runtime for g++ in this image")
    assert r.returncode == 0, r.stderr.decode()[-3000:]

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"),
                           timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        return r.stdout.decode()
    return run


def from_bits(words):
    return np.array([int(w, 16) for w in words], np.uint64).view(np.float64)


def ulps(a, b):
    """distance in units of the last place between same-signed doubles"""
    return np.abs(a.view(np.int64) - b.view(np.int64))


# ---- Philox ---------------------------------------------------------------------------------------------------------------

def test_philox_known_answers_library_and_reference(harness):
    assert harness("kat").split("\n")[:3] == KATS
    for (c, k), want in zip(KAT_INPUTS, KATS):
        assert " ".join("%08x" % int(x[0]) for x in R.philox(*c, *k)) == want
    # vectorised counters give what one counter at a time gives
    idx = np.arange(50)
    many = R.philox(idx, 3, 5, 0, 17, 4)
    for i in (0, 7, 49):
        assert [int(x[i]) for x in many] == [int(x[0]) for x in R.philox(i, 3, 5, 0, 17, 4)]


# ---- the derived variates: library against reference --------------------------------------------------------------------------

def test_normal_of_the_library_is_the_references(harness):
    """2000 counters: libm and numpy may differ in the last bits of log / cos — 4 ulp."""
    seed = 20261019
    lib = from_bits(harness("normal", seed, 2000).split())
    ref = R.normal(seed, np.arange(2000), 3, 5, 0)
    assert len(lib) == 2000 and (np.sign(lib) == np.sign(ref)).all()
    assert ulps(lib, ref).max() <= 4, ulps(lib, ref).max()
    assert len(np.unique(lib)) == 2000


@pytest.mark.parametrize("shape", [1.0, 1.5, 300.5])
def test_gamma_of_the_library_is_the_references(harness, shape):
    """2000 draws a shape: the same number of attempts, the values to 4 ulp."""
    seed, rate = 7, 20.0
    rows = [ln.split() for ln in harness("gamma", seed, shape, rate, 2000).strip().split("\n")]
    lib, attempts = from_bits([r[0] for r in rows]), np.array([int(r[1]) for r in rows])
    ref = [R.gamma(seed, 1, t, R.STREAM_LAMBDA, shape, rate) for t in range(2000)]
    assert np.array_equal(attempts, [a for _, a in ref])
    assert ulps(lib, np.array([g for g, _ in ref])).max() <= 4
    if shape == 1.0:
        assert attempts.max() > 1           # the rejection path was taken


# ---- moments (fixed seeds: deterministic) -----------------------------------------------------------------------------------

def test_moments_of_the_normal(harness):
    """20,000 normals: |mean| within 5 / sqrt(n), |var - 1| within 5 sqrt(2 / n) (the standard errors of a unit normal's mean and variance)."""
    n = 20000
    z = from_bits(harness("normal", 12345, n).split())
    assert abs(z.mean()) <= 5.0 / np.sqrt(n), z.mean()
    assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n), z.var()
    zr = R.normal(99, np.arange(n), 1, 2, 0)
    assert abs(zr.mean()) <= 5.0 / np.sqrt(n) and abs(zr.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)


@pytest.mark.parametrize("shape", [1.0, 1.5, 300.5])
def test_moments_of_the_gamma(harness, shape):
    """4000 gammas: the mean within 5 standard errors of a / rate; the variance within 5 standard errors of a / rate^2 — the sample
    variance of a Gamma(a) has variance (mu_4 - sigma^4) / n with mu_4 = 3 a (a + 2) / rate^4."""
    n, rate = 4000, 20.0
    g = from_bits([ln.split()[0] for ln in harness("gamma", 31, shape, rate, n).strip().split("\n")])
    mean, var = shape / rate, shape / rate ** 2
    assert abs(g.mean() - mean) <= 5.0 * np.sqrt(var / n), (g.mean(), mean)
    mu4 = 3.0 * shape * (shape + 2.0) / rate ** 4
    assert abs(g.var() - var) <= 5.0 * np.sqrt((mu4 - var ** 2) / n), (g.var(), var)


def test_host_arithmetic_under_the_sanitizers(harness):
    """Seeded draws of every kind, m = 0, a shape whose gamma needs more than one attempt, a shape below 1, the settings' validation."""
    for seed in (20261019, 5):
        assert "checks ok" in harness("check", seed)


# ---- symbols -------------------------------------------------------------------------------------------------------------

def test_header_matches_the_binding():
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_mcmc.h")).read()
    declared = set(re.findall(r"\b(fmhip_mcmc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_MCMC) == {"fmhip_mcmc_" + n for n in ("opts_default", "create", "destroy", "epoch", "get_state", "set_state",
                                                                              "reset_average", "predictions")}
    others = (_ffi.SYMBOLS + _ffi.SYMBOLS_EXPERIMENTAL + _ffi.SYMBOLS_TOPK + _ffi.SYMBOLS_PAIRING + _ffi.SYMBOLS_METRICS + _ffi.SYMBOLS_RANKING
              + _ffi.SYMBOLS_WEIGHTS + _ffi.SYMBOLS_RELATIONAL)
    assert not set(_ffi.SYMBOLS_MCMC) & set(others)
    L = _ffi.load()
    for name in _ffi.SYMBOLS_MCMC:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert "fmhip_mcmc.hip" in _build.HIP_SOURCES and "mcmc_rng.h" in _build.HIP_DEPS and any(d.endswith("fmhip_mcmc.h") for d in _build.HIP_DEPS)
    assert "mcmc" not in open(os.path.join(ROOT, "include", "fmhip.h")).read()               # fmhip.h stays as it is
    # the struct the binding passes is the header's
    fields = re.search(r"typedef struct \{(.*?)\} fmhip_mcmc_opts;", hdr, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [n for n, _ in _ffi.McmcOpts._fields_]
    o = _ffi.McmcOpts()
    assert L.fmhip_mcmc_opts_default(C.byref(o)) == 0
    assert (o.seed, o.sample, o.reg0, o.init_lambda, o.alpha_0, o.beta_0, o.alpha_lambda, o.beta_lambda, o.gamma_0, o.mu_0) == (0, 1, 0.0, 1.0, 1, 1, 1, 1, 1, 0)
    import sparkfm_amd
    assert issubclass(sparkfm_amd.HipMCMC, sparkfm_amd.FMLearn) and "HipMCMC" in sparkfm_amd.__all__


# ---- refusals that need no device ----------------------------------------------------------------------------------------------

def test_c_calls_refuse_null_handles_and_bad_priors_without_a_device():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    h = C.c_void_p(7)
    assert L.fmhip_mcmc_opts_default(None) == -1 and b"opts is NULL" in L.fmhip_last_error()
    assert L.fmhip_mcmc_create(None, None, None, None, None) == -1 and b"out is NULL" in L.fmhip_last_error()
    assert L.fmhip_mcmc_create(None, None, None, None, C.byref(h)) == -1 and h.value is None and b"model or train set is NULL" in L.fmhip_last_error()
    for name, bad in (("alpha_0", 0.0), ("beta_0", -1.0), ("alpha_lambda", float("nan")), ("beta_lambda", float("inf")), ("gamma_0", 0.0),
                      ("mu_0", float("inf")), ("reg0", -0.5), ("init_lambda", 0.0)):
        o = _ffi.McmcOpts()
        L.fmhip_mcmc_opts_default(C.byref(o))
        setattr(o, name, bad)
        assert L.fmhip_mcmc_create(None, None, None, C.byref(o), C.byref(h)) == -1 and name.encode() in L.fmhip_last_error(), name
    assert L.fmhip_mcmc_destroy(None) == 0
    assert L.fmhip_mcmc_epoch(None, None) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_mcmc_get_state(None, None, None, None, None) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_mcmc_set_state(None, 1.0, None, None) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_mcmc_reset_average(None) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_mcmc_predictions(None, None, None, None) == -1 and b"NULL" in L.fmhip_last_error()


def test_hipmcmc_validates_its_arguments():
    from sparkfm_amd import DataSet, HipMCMC, Relation, RelationalData
    m = HipMCMC.run()
    assert (m.seed, m.burn_in, m.sample, m.test) == (0, 0, True, None) and m.priors["alpha_0"] == 1.0 and m.priors["reg0"] == 0.0
    m = HipMCMC.run(seed=2 ** 40 + 3, burn_in=15, sample=False, gamma_0=2.5, mu_0=-1.0, reg0=0.0)
    assert (m.seed, m.burn_in, m.sample) == (2 ** 40 + 3, 15, False) and m.priors["gamma_0"] == 2.5 and m.priors["mu_0"] == -1.0
    for kw, exc in ((dict(seed=-1), ValueError), (dict(seed=2 ** 64), ValueError), (dict(seed=1.5), TypeError), (dict(burn_in=-1), ValueError),
                    (dict(sample=1), ValueError), (dict(alpha_0=0.0), ValueError), (dict(beta_lambda=float("nan")), ValueError),
                    (dict(reg0=-1.0), ValueError), (dict(init_lambda=float("inf")), ValueError), (dict(lam=1.0), TypeError)):
        with pytest.raises(exc):
            HipMCMC.run(**kw)
    with pytest.raises(ValueError, match="scoring"):
        HipMCMC.run(test=DataSet(np.zeros(2, np.int64) + [0, 1], [0], [1.0], [1.0], scoring=True))
    rd = RelationalData([1.0, 2.0], [Relation([([1], [1.0]), ([2], [1.0])], [0, 1])])
    with pytest.raises(TypeError, match="RelationalData.*expand"):
        HipMCMC.run(test=rd)
    # no handle before the first learn; a RelationalData is answered as by the other non-relational calls, before any device call
    for call in (lambda: m.state, m.reset_average, lambda: HipMCMC.run(test=DataSet([0, 1], [0], [1.0], [1.0])).predictions()):
        with pytest.raises(RuntimeError, match="first learn"):
            call()
    with pytest.raises(RuntimeError, match="without a test set"):
        m.predictions()
    from sparkfm_amd import FMModel
    fm = FMModel(2, 2)
    fm._h, fm._dev_fresh = C.c_void_p(1), True                  # (no device: the handle is never used)
    try:
        with pytest.raises(TypeError, match="RelationalData.*expand"):
            m.learn(fm, rd)
    finally:
        fm._h = None
