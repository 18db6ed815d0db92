"""The MCMC learner over relational data, host surface (no GPU): the header against the binding and the build lists, the refusals that
need no device, HipMCMC's validation, the fp64 twin by block caches (mcmc_blocks_ref.py) pinned to the flat twins on the expanded rows,
and the host passes of the sweep (csrc/fmhip_host.cpp: mcmc_part_order, mcmc_block_counts, mcmc_block_trained, driven by
tests/host_mcmc_relational_harness.cpp — a stand-alone program built with AddressSanitizer and UBSan)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import mcmc_blocks_cases as K
import mcmc_blocks_ref as B
import mcmc_ref as R
import probit_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_matches_the_binding_and_the_build():
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_mcmc_relational.h")).read()
    declared = set(re.findall(r"\b(fmhip_mcmc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_MCMC_RELATIONAL) == {"fmhip_mcmc_create_relational"}
    others = (_ffi.SYMBOLS + _ffi.SYMBOLS_EXPERIMENTAL + _ffi.SYMBOLS_TOPK + _ffi.SYMBOLS_PAIRING + _ffi.SYMBOLS_METRICS + _ffi.SYMBOLS_RANKING
              + _ffi.SYMBOLS_WEIGHTS + _ffi.SYMBOLS_RELATIONAL + _ffi.SYMBOLS_MCMC + _ffi.SYMBOLS_MCMC_TASK + _ffi.SYMBOLS_MCMC_GROUPS + _ffi.SYMBOLS_BPR)
    assert not set(_ffi.SYMBOLS_MCMC_RELATIONAL) & set(others)
    L = _ffi.load()
    fn = L.fmhip_mcmc_create_relational
    assert len(fn.argtypes) == 8 and fn.restype is C.c_int
    assert "fmhip_mcmc_relational.hip" in _build.HIP_SOURCES and os.path.exists(os.path.join(_build.CSRC, "fmhip_mcmc_relational.hip"))
    for dep in ("mcmc_blocks.h", "fmhip_mcmc_handle.h"):
        assert dep in _build.HIP_DEPS and os.path.exists(os.path.join(_build.CSRC, dep))
    assert any(d.endswith("fmhip_mcmc_relational.h") for d in _build.HIP_DEPS)
    # the older headers keep their declarations; fmhip_mcmc.h's closing comment points here, and so does sparkfm.hpp
    for name, symbols in (("fmhip_mcmc.h", _ffi.SYMBOLS_MCMC), ("fmhip_mcmc_task.h", _ffi.SYMBOLS_MCMC_TASK), ("fmhip_mcmc_groups.h", _ffi.SYMBOLS_MCMC_GROUPS)):
        text = open(os.path.join(ROOT, "include", name)).read()
        assert set(re.findall(r"\b(fmhip_mcmc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))) == set(symbols)
    assert "fmhip_mcmc_relational.h" in open(os.path.join(ROOT, "include", "fmhip_mcmc.h")).read()
    assert "fmhip_mcmc_create_relational" in open(os.path.join(ROOT, "include", "sparkfm.hpp")).read()
    assert int(re.search(r"#define FMHIP_RELATIONS_MAX (\d+)", open(os.path.join(ROOT, "include", "fmhip_relational.h")).read()).group(1)) == 8


def test_refusals_that_need_no_device():
    from sparkfm_amd import DataSet, FMModel, HipBlockMCMC, HipMCMC, Relation, RelationalData, _ffi
    L = _ffi.load()
    h = C.c_void_p()
    assert L.fmhip_mcmc_create_relational(None, None, None, None, None, None, 0, None) == -1 and b"out is NULL" in L.fmhip_last_error()
    assert L.fmhip_mcmc_create_relational(None, None, None, None, None, None, 0, C.byref(h)) == -1 and b"model or train set is NULL" in L.fmhip_last_error()
    bad = _ffi.McmcOpts(0, 1, 0.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 0.0)         # alpha_0 = 0
    assert L.fmhip_mcmc_create_relational(None, None, None, None, C.byref(bad), None, 1, C.byref(h)) == -1 and b"alpha_0" in L.fmhip_last_error()
    task = _ffi.McmcTaskOpts(_ffi.MCMC_CLASSIFICATION, 1, 0.0, 1.0)
    assert L.fmhip_mcmc_create_relational(None, None, None, None, None, C.byref(task), 0, C.byref(h)) == -1 and b"clip" in L.fmhip_last_error()
    assert h.value is None
    # the texts the library refuses with, where they are written
    src = open(os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_mcmc_relational.hip")).read()
    for words in ("lies inside the id range of", "batches: the MCMC learner walks whole blocks", "at most one of the two", "%s, %s: %s"):
        assert words in src, words
    assert "its attribute groups are its parts" in open(os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_mcmc.hip")).read()
    # HipBlockMCMC: 'parts' and a relational test set are taken, anything else named by a string is not; HipMCMC takes neither
    import sparkfm_amd
    assert issubclass(HipBlockMCMC, HipMCMC) and "HipBlockMCMC" in sparkfm_amd.__all__
    rd = RelationalData([1.0, 2.0], [Relation([([1], [1.0]), ([2], [1.0])], [0, 1])])
    m = HipBlockMCMC.run(groups="parts", test=rd)
    assert m.groups == "parts" and m.test is rd and HipBlockMCMC.run().groups is None
    with pytest.raises(TypeError, match="'parts'"):
        HipBlockMCMC.run(groups="fields")
    with pytest.raises(TypeError, match="'parts'"):
        HipMCMC.run(groups="parts")
    with pytest.raises(TypeError, match="RelationalData.*expand"):
        HipMCMC.run(test=rd)
    fm = FMModel(2, 2)
    fm._h, fm._dev_fresh = C.c_void_p(1), True                  # (no device: the handle is never used)
    try:
        flat = DataSet([0, 1], [0], [1.0], [1.0])
        with pytest.raises(TypeError, match="sweeps the blocks of a RelationalData"):
            m.learn(fm, flat)
        with pytest.raises(TypeError, match="RelationalData.*expand"):
            HipMCMC.run().learn(fm, rd)
        for groups in (np.zeros(3, np.int32), rd.meta()):
            with pytest.raises(ValueError, match="groups='parts'"):
                HipBlockMCMC.run(groups=groups).learn(fm, rd)
    finally:
        fm._h = None
    with pytest.raises(TypeError, match="HipBlockMCMC.learn"):
        rd.handle
    assert "HipBlockMCMC.learn" in RelationalData.__doc__


@pytest.mark.parametrize("by_parts,task,sample", K.CASES, ids=K.IDS)
def test_the_block_twin_is_the_flat_twin_on_the_expanded_rows(by_parts, task, sample):
    """3 epochs of mcmc_blocks_ref on base_problem against mcmc_groups_ref (+ probit_ref's targets) on expand(): w, v, w0, alpha,
    lambda, mu and the test predictions.  Measured here (fp64 numpy): every quantity within 2e-15 except mu by parts 4.9e-14, w0 under
    the probit link 1.9e-14 and the predictions 5.3e-15 — mcmc_blocks_cases.RECORDED holds the figures per case, and this test holds
    the twins to them; 1e-10 separates either from a wrong term."""
    prob = B.base_problem(K.SEED, classification=task == "classification")
    a, b = K.run_blocks(prob, by_parts, task, sample), K.run_flat(prob, by_parts, task, sample)
    flat_test = prob["test"].expand()
    pa, pb = B.predict(a, prob["test"]), R.predict(b.w0, b.w, b.v, flat_test)
    if task == "classification":
        pa, pb = PR.normal_cdf(pa), PR.normal_cdf(pb)
    d = K.distances(a, b, pa, pb)
    print({name: "%.2e" % value for name, value in d.items()})
    assert np.abs(a.w - prob["w"]).max() > 0.1 and np.abs(a.v - prob["v"]).max() > 0.01         # both moved
    for name in K.QUANTITIES:
        assert d[name] <= K.RECORDED[(by_parts, task, sample)][name], (name, d[name])
    # T: the feature of the rows nobody references and those rows' ids are not trained, nor is quirk Q1's slot
    n1 = prob["n1"]
    counts = B.group_counts(prob["train"], n1 - 1)
    assert counts.sum() == int((prob["train"].expand().feat < n1 - 1).sum())
    for i in (B.USERS - 2, B.USERS - 1, prob["lonely"], n1 - 1):
        assert a.w[i] == prob["w"][i] and b.w[i] == prob["w"][i]


def test_the_problem_has_the_shapes_the_sweep_can_go_wrong_at():
    prob = B.base_problem(K.SEED)
    users, items, plain = prob["train"].parts
    assert (users.n_rows, items.n_rows, prob["train"].n_rows) == (40, 25, 300) and plain.mapping is None
    n = B.counts(prob["train"], users)
    assert n[-2:].tolist() == [0.0, 0.0] and (n[:-2] >= 0).all()
    lonely = prob["lonely"]
    assert set(users.crow[users.cptr[list(users.feat).index(lonely)]:users.cptr[list(users.feat).index(lonely) + 1]]) == {38, 39}
    lens = np.diff(users.row_ptr)
    assert lens.min() >= 3 and lens.max() <= 6 and np.diff(items.row_ptr).min() == 2 and np.diff(items.row_ptr).max() == 3
    # contiguous, disjoint id ranges in the order users < items < plain; the last id is num_attribute
    assert users.feat.max() < items.feat.min() and items.feat.max() < plain.feat.min() and plain.feat.max() == prob["n1"] - 1
    big = B.base_problem(K.SEED, n_rows=700)
    assert np.bincount(big["train"].parts[1].mapping).max() > 256
    assert prob["train"].order == [0, 1, 2]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mcmc_relational") / "host_mcmc_relational_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "host_mcmc_relational_harness.cpp"), os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_host.cpp"), "-o", exe]
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


def test_the_host_passes_under_the_sanitizers(harness):
    """The parts' order (given in any order; parts without features; interleaved, nested and touching ranges named), n_p, and the
    trained columns (quirk Q1's slot, empty columns, columns that live only in rows nobody references, the row words' flag bit),
    on the edge cases and 200 random shapes a seed."""
    for seed in (1, 2, 3):
        assert "checks ok" in harness("check", seed)
