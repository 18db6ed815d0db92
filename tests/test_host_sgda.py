"""The SGDA learner, host surface (no GPU): the header against the binding and the library, the refusals that need no device,
HipSGDA's validation of its keywords, the host plan of the grouped sums (csrc/fmhip_host.cpp: sgda_group_plan, driven by
tests/host_sgda_harness.cpp — a stand-alone program built with AddressSanitizer and UBSan), and the fp64 twin (sgda_ref.py) on the
planted task: what adaptive per-group regularisation buys over the best fixed lambda."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sgda_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("create", "destroy", "step", "epoch", "get_lambda", "set_lambda", "last_sums", "info")


# ---- symbols ---------------------------------------------------------------------------------------------------------------

def test_header_matches_the_binding():
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_sgda.h")).read()
    declared = set(re.findall(r"\b(fmhip_sgda_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_SGDA) == {"fmhip_sgda_" + n for n in NAMES}
    others = (_ffi.SYMBOLS + _ffi.SYMBOLS_EXPERIMENTAL + _ffi.SYMBOLS_TOPK + _ffi.SYMBOLS_PAIRING + _ffi.SYMBOLS_METRICS + _ffi.SYMBOLS_RANKING
              + _ffi.SYMBOLS_WEIGHTS + _ffi.SYMBOLS_RELATIONAL + _ffi.SYMBOLS_MCMC + _ffi.SYMBOLS_MCMC_TASK + _ffi.SYMBOLS_MCMC_GROUPS
              + _ffi.SYMBOLS_MCMC_RELATIONAL + _ffi.SYMBOLS_BPR + _ffi.SYMBOLS_BPR_ADAPTIVE + _ffi.SYMBOLS_WARP + _ffi.SYMBOLS_FTRL + _ffi.SYMBOLS_REDRAW)
    assert not set(_ffi.SYMBOLS_SGDA) & set(others)
    core = open(os.path.join(ROOT, "include", "fmhip.h")).read()          # fmhip.h keeps its entry points, and none of these
    assert set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", core, flags=re.S))) == set(_ffi.SYMBOLS)
    L = _ffi.load()
    for name in _ffi.SYMBOLS_SGDA:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert int(re.search(r"#define FMHIP_SGDA_MAX_GROUPS (\d+)", hdr).group(1)) == _ffi.SGDA_MAX_GROUPS == 4096
    assert any(d.endswith("fmhip_sgda.h") for d in _build.HIP_DEPS) and "fm_sgda.h" in _build.HIP_DEPS
    assert "fm_sgda.hip" in _build.HIP_SOURCES and "fmhip_sgda.hip" in _build.HIP_SOURCES
    # the MCMC groups' header no longer lists the SGD learners as missing
    groups = open(os.path.join(ROOT, "include", "fmhip_mcmc_groups.h")).read()
    assert "regularisation of the SGD learners" not in groups and "fmhip_sgda.h" in groups
    import sparkfm_amd
    assert "HipSGDA" in sparkfm_amd.__all__ and issubclass(sparkfm_amd.HipSGDA, sparkfm_amd.HipSGD)


def test_header_compiles_as_plain_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "fmhip_sgda.h"\nint main(void) { fmhip_sgda_t h = 0; return fmhip_sgda_destroy(h) + (FMHIP_SGDA_MAX_GROUPS != 4096); }\n')
    lib = os.path.join(ROOT, "sparkfm_amd", "lib")
    exe = str(tmp_path / "use")
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe,
                    "-L", lib, "-lfmhip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"], check=True)
    assert subprocess.run([exe]).returncode == 0          # destroying a NULL handle is fine


# ---- refusals that need no device -----------------------------------------------------------------------------------------

def test_c_calls_refuse_without_a_device():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    table = np.zeros(4, np.int32)
    h = C.c_void_p()
    err = L.fmhip_last_error
    assert L.fmhip_sgda_create(None, _ffi.ptr(table), 4, 1, 0.0, 0.0, None) == -1 and b"out is NULL" in err()
    assert L.fmhip_sgda_create(None, None, 4, 1, 0.0, 0.0, C.byref(h)) == -1 and b"group table is NULL" in err()
    assert L.fmhip_sgda_create(None, _ffi.ptr(table), 4, 0, 0.0, 0.0, C.byref(h)) == -1 and b"n_groups = 0" in err()
    assert L.fmhip_sgda_create(None, _ffi.ptr(table), 4, -2, 0.0, 0.0, C.byref(h)) == -1 and b"n_groups = -2" in err()
    assert L.fmhip_sgda_create(None, _ffi.ptr(table), 4, 4097, 0.0, 0.0, C.byref(h)) == -5 and b"FMHIP_SGDA_MAX_GROUPS" in err()
    for lw, lv in ((-1.0, 0.0), (0.0, -1e-9), (float("nan"), 0.0), (0.0, float("inf"))):
        assert L.fmhip_sgda_create(None, _ffi.ptr(table), 4, 2, lw, lv, C.byref(h)) == -1 and b"finite and >= 0" in err()
    assert L.fmhip_sgda_create(None, _ffi.ptr(table), 4, 4096, 0.0, 0.0, C.byref(h)) == -1 and b"model is NULL" in err()
    assert h.value is None
    assert L.fmhip_sgda_destroy(None) == 0
    assert L.fmhip_sgda_step(None, None, 0, None, 0, 0.1, 0.1, 0.0, None, None) == -1 and b"handle is NULL" in err()
    assert L.fmhip_sgda_epoch(None, None, None, 0.1, 0.1, 0.0, None, None, None) == -1 and b"handle is NULL" in err()
    assert L.fmhip_sgda_get_lambda(None, None, None) == -1 and b"handle is NULL" in err()
    assert L.fmhip_sgda_set_lambda(None, None, None) == -1 and b"handle is NULL" in err()
    assert L.fmhip_sgda_last_sums(None, None, None) == -1 and b"handle is NULL" in err()
    assert L.fmhip_sgda_info(None, None, None, None) == -1 and b"handle is NULL" in err()


def test_hipsgda_validates_its_keywords():
    from sparkfm_amd import DataSet, FMModel, HipSGDA, Metadata, RelationalData, Relation, _ffi
    val = DataSet([0, 1], [0], [1.0], [1.0])
    s = HipSGDA.run(validation=val)
    assert s.eta == 0.05 and s.eta_lambda == s.eta and s.groups is None and s.n_groups == 1 and s.init_lambda == 0.0          # libFM's choice
    assert s.optimizer == "sgd" and s.pairs is False and s.regw == 0.0 and s.regv == 0.0
    s = HipSGDA.run(validation=val, groups=Metadata.fromFields((2, 0, 1)), eta=0.1, eta_lambda=0.5, loss="logistic")
    assert s.groups.tolist() == [0, 0, 2] and s.n_groups == 3 and s.eta_lambda == 0.5 and s.loss == "logistic"
    assert HipSGDA.run(validation=val, groups=[0, 4095]).n_groups == 4096
    for kw, exc in ((dict(groups=[0, -1]), ValueError), (dict(groups=[0.0, 1.0]), TypeError), (dict(groups=[[0, 1]]), TypeError),
                    (dict(groups=[0, 4096]), ValueError), (dict(eta_lambda=-1.0), ValueError), (dict(init_lambda=-0.5), ValueError),
                    (dict(init_lambda=float("nan")), ValueError), (dict(loss="hinge"), ValueError),
                    (dict(init_lambda=([0.0], [[0.0]])), ValueError)):          # a pair goes with fixed regularisation only
        with pytest.raises(exc):
            HipSGDA.run(validation=val, **kw)
    with pytest.raises(ValueError, match="needs a validation set"):
        HipSGDA.run()                                                           # eta_lambda defaults to eta
    with pytest.raises(ValueError, match="scoring=True"):
        HipSGDA.run(validation=DataSet([0, 1], [0], [1.0], [1.0], scoring=True))
    fixed = HipSGDA.run(eta_lambda=0, groups=[0, 1, 1], init_lambda=([0.1, 0.2], [[0.3, 0.4]]))
    assert fixed.validation is None and fixed.eta_lambda == 0.0
    for what in ("state", "group_counts"):
        with pytest.raises(RuntimeError, match="first learn"):
            getattr(fixed, what)
    with pytest.raises(RuntimeError, match="first learn"):
        fixed.last_sums()
    # a table of the wrong length raises when the handle is made, before any device call; so does relational data
    fm = FMModel(6, 2)
    fm._h, fm._dev_fresh = C.c_void_p(1), True                  # (no device: the handle is never used)
    ds = DataSet([0, 1], [0], [1.0], [1.0])
    ds._h = C.c_void_p(2)
    try:
        with pytest.raises(ValueError, match="groups holds 3 ids but the model has num_attribute \\+ 1 = 7"):
            fixed._handle(fm)
        rd = RelationalData([1.0], [Relation([([0], [1.0])], [0])])
        with pytest.raises(_ffi.FmhipError) as e:
            fixed.learn(fm, rd)
        assert e.value.code == -5
    finally:
        fm._h, ds._h = None, None


# ---- the host plan under the sanitizers --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sgda") / "host_sgda_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "host_sgda_harness.cpp"), os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_host.cpp"), "-o", exe]
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


def test_the_chunk_plan_under_the_sanitizers(harness):
    """G = 1; G = 3 with interleaved ids; a group of exactly the chunk length, one of chunk length + 1 and one with no feature in one
    table; no feature at all; 300 random shapes a seed: every id in exactly one chunk, chunks in group order that never straddle a
    group or exceed the chunk length, ids ascending inside a group, no chunk for an empty group, the counts right."""
    for seed in (20261021, 9):
        assert "checks ok" in harness("check", seed)


# ---- the twin on the planted task ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted_runs():
    out = {}
    for seed in sref.SEEDS:
        t = sref.planted(seed)
        one = np.zeros(t["n1"], np.int32)
        fixed = [sref.run_planted(t, one, 1, 0.0, lam, validation=False)[2] for lam in sref.FIXED]
        out[seed] = dict(task=t, fixed=fixed, two=sref.run_planted(t, t["group"], 2, sref.ETA_LAMBDA), one=sref.run_planted(t, one, 1, sref.ETA_LAMBDA))
    return out


@pytest.mark.parametrize("seed", sref.SEEDS)
def test_two_groups_beat_the_best_fixed_lambda(planted_runs, seed):
    """The README's table: with an informative and a noise group the adapted regularisers beat every lambda of the grid on the test
    set, the noise group's lambda_w ends above the informative group's, and no lambda is negative."""
    r = planted_runs[seed]
    s, val, test = r["two"]
    print("seed %d: fixed %s; two groups: test %.4f, validation %.4f, lambda_w %s, lambda_v %s; one group: test %.4f, lambda_w %s" % (
        seed, ["%.4f" % x for x in r["fixed"]], test, val, s.lw.round(4).tolist(), s.lv.round(3).tolist(), r["one"][2], r["one"][0].lw.round(4).tolist()))
    assert test < min(r["fixed"])
    assert s.lw[1] > s.lw[0]
    assert (s.lw >= 0).all() and (s.lv >= 0).all() and (r["one"][0].lw >= 0).all() and (r["one"][0].lv >= 0).all()
    assert np.isfinite(val) and s.steps == sref.EPOCHS * (sref.N_TRAIN // sref.BATCH)


@pytest.mark.parametrize("loss", ["squared", "logistic"])
def test_without_adaptation_the_twin_is_plain_sgd(loss):
    """eta_lambda = 0, with or without a validation set, G = 1 or 3 groups that share one lambda: the twin's parameters EQUAL plain
    fp64 mini-batch SGD with regw = regv = init_lambda, written out on its own."""
    t = sref.planted(3, loss)
    X, y = t["train"]
    lam = 0.03
    w0, w, v = t["w0"], t["w"].copy(), t["v"].copy()
    states = [sref.State(w0, w, v, 1, lam, lam), sref.State(w0, w, v, 3, lam, lam), sref.State(w0, w, v, 1, lam, lam)]
    groups = [np.zeros(t["n1"], np.int32), np.arange(t["n1"], dtype=np.int32) % 3, np.zeros(t["n1"], np.int32)]
    for _ in range(3):
        w0, w, v = sref.sgd_epoch(w0, w, v, X, y, sref.BATCH, sref.ETA, 0.01, lam, lam, loss)
        for j, (s, g) in enumerate(zip(states, groups)):
            sref.epoch(s, g, X, y, t["val"][0] if j == 2 else None, t["val"][1], sref.BATCH, sref.ETA, 0.0, 0.01, loss)
    for s in states:
        assert s.w0 == w0 and np.array_equal(s.w, w) and np.array_equal(s.v, v)
        assert (s.lw == lam).all() and (s.lv == lam).all()
