"""The MCMC learner's attribute groups, host surface (no GPU): the header against the binding, the refusals that need no device,
Metadata's arithmetic, HipMCMC's validation of `groups`, and the host plan of the grouped sums (csrc/fmhip_host.cpp: mcmc_group_plan)
and the epoch's hyper-parameter draws (csrc/fmhip_host.h: mcmc_draw_state), both driven by tests/host_mcmc_groups_harness.cpp — a
stand-alone program built with AddressSanitizer and UBSan."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- symbols ---------------------------------------------------------------------------------------------------------------

def test_header_matches_the_binding():
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_mcmc_groups.h")).read()
    declared = set(re.findall(r"\b(fmhip_mcmc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_MCMC_GROUPS) == {"fmhip_mcmc_" + n for n in ("set_groups", "group_info", "get_group_state", "set_group_state")}
    others = (_ffi.SYMBOLS + _ffi.SYMBOLS_EXPERIMENTAL + _ffi.SYMBOLS_TOPK + _ffi.SYMBOLS_PAIRING + _ffi.SYMBOLS_METRICS + _ffi.SYMBOLS_RANKING
              + _ffi.SYMBOLS_WEIGHTS + _ffi.SYMBOLS_RELATIONAL + _ffi.SYMBOLS_MCMC + _ffi.SYMBOLS_MCMC_TASK)
    assert not set(_ffi.SYMBOLS_MCMC_GROUPS) & set(others)
    L = _ffi.load()
    for name in _ffi.SYMBOLS_MCMC_GROUPS:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    assert int(re.search(r"#define FMHIP_MCMC_MAX_GROUPS (\d+)", hdr).group(1)) == _ffi.MCMC_MAX_GROUPS == 4096
    assert any(d.endswith("fmhip_mcmc_groups.h") for d in _build.HIP_DEPS)
    # the older headers keep their declarations: only fmhip_mcmc.h's closing comment points here
    for name, symbols in (("fmhip_mcmc.h", _ffi.SYMBOLS_MCMC), ("fmhip_mcmc_task.h", _ffi.SYMBOLS_MCMC_TASK)):
        text = open(os.path.join(ROOT, "include", name)).read()
        assert set(re.findall(r"\b(fmhip_mcmc_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S))) == set(symbols)
    assert "fmhip_mcmc_groups.h" in open(os.path.join(ROOT, "include", "fmhip_mcmc.h")).read()
    import sparkfm_amd
    assert "Metadata" in sparkfm_amd.__all__ and sparkfm_amd.Metadata is sparkfm_amd.metadata.Metadata


# ---- refusals that need no device -----------------------------------------------------------------------------------------

def test_c_calls_refuse_without_a_device():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    table = np.zeros(4, np.int32)
    assert L.fmhip_mcmc_set_groups(None, None, 4, 1) == -1 and b"group table is NULL" in L.fmhip_last_error()
    assert L.fmhip_mcmc_set_groups(None, _ffi.ptr(table), 4, 0) == -1 and b"n_groups = 0" in L.fmhip_last_error()
    assert L.fmhip_mcmc_set_groups(None, _ffi.ptr(table), 4, -3) == -1 and b"n_groups = -3" in L.fmhip_last_error()
    assert L.fmhip_mcmc_set_groups(None, _ffi.ptr(table), 4, 4097) == -5 and b"FMHIP_MCMC_MAX_GROUPS" in L.fmhip_last_error()
    assert L.fmhip_mcmc_set_groups(None, _ffi.ptr(table), 4, 4096) == -1 and b"handle is NULL" in L.fmhip_last_error()
    assert L.fmhip_mcmc_group_info(None, None, None) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_mcmc_get_group_state(None, None, None, None, None) == -1 and b"NULL" in L.fmhip_last_error()
    assert L.fmhip_mcmc_set_group_state(None, 1.0, None, None) == -1 and b"NULL" in L.fmhip_last_error()


# ---- Metadata --------------------------------------------------------------------------------------------------------------

def test_metadata_arithmetic():
    from sparkfm_amd import Metadata
    m = Metadata(5)
    assert m.attrGroup.tolist() == [0] * 5 and m.numAttrGroups == 1 and m.numAttrPerGroup.tolist() == [5]          # the reference's start
    assert m.update([0, 2, 2, 0, 2]) is m
    assert m.numAttrGroups == 3 and m.numAttrPerGroup.tolist() == [2, 0, 3] and m.attrGroup.dtype == np.int32        # max + 1, an empty group
    assert m.update([1, 1, 1, 1, 1]).numAttrPerGroup.tolist() == [0, 5]
    assert m.update([0, 0, 0, 0, 0], numAttrGroups=4).numAttrPerGroup.tolist() == [5, 0, 0, 0]
    assert m.numAttrPerGroup.sum() == m.dimension
    for bad, exc in (([0, 1], ValueError), ([0, 1, -1, 0, 0], ValueError), ([0.5] * 5, TypeError), ([[0] * 5], ValueError)):
        with pytest.raises(exc):
            m.update(bad)
    with pytest.raises(ValueError, match="names group 2"):
        m.update([0, 1, 2, 0, 0], numAttrGroups=2)
    with pytest.raises(ValueError):
        Metadata(-1)
    e = Metadata(0)
    assert e.numAttrGroups == 1 and e.numAttrPerGroup.tolist() == [0] and e.update([]).numAttrGroups == 1
    f = Metadata.fromFields((3, 0, 2))
    assert f.dimension == 5 and f.attrGroup.tolist() == [0, 0, 0, 2, 2] and f.numAttrGroups == 3 and f.numAttrPerGroup.tolist() == [3, 0, 2]
    f = Metadata.fromFields((2, 3), dimension=7)
    assert f.attrGroup.tolist() == [0, 0, 1, 1, 1, 1, 1] and f.numAttrPerGroup.tolist() == [2, 5]
    with pytest.raises(ValueError):
        Metadata.fromFields((4, 4), dimension=7)
    with pytest.raises(ValueError):
        Metadata.fromFields(())


def test_relational_meta_names_a_group_per_part():
    from sparkfm_amd import DataSet, Relation, RelationalData
    users = Relation([([0], [1.0]), ([1, 2], [1.0, 0.5])], [0, 1, 1])
    items = Relation([([4], [1.0]), ([5], [1.0]), ([6], [2.0])], [2, 0, 1])
    plain = DataSet([0, 1, 2, 3], [8, 9, 8], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0])
    rd = RelationalData([1.0, 2.0, 3.0], [users, items], plain=plain)
    meta = rd.meta()
    assert meta.dimension == rd.dimension == 9 and meta.numAttrGroups == 3
    assert meta.attrGroup.tolist() == [0, 0, 0, 0, 1, 1, 1, 0, 2]        # ids 3 and 7 are unused: group 0; id 9 is the spare slot
    assert RelationalData([1.0, 2.0, 3.0], [users, items]).meta().numAttrGroups == 2


# ---- HipMCMC ---------------------------------------------------------------------------------------------------------------

def test_hipmcmc_validates_groups():
    from sparkfm_amd import FMModel, HipMCMC, Metadata
    m = HipMCMC.run()
    assert m.groups is None and m.n_groups == 1
    m = HipMCMC.run(groups=[0, 1, 1, 3])
    assert m.groups.tolist() == [0, 1, 1, 3] and m.groups.dtype == np.int32 and m.n_groups == 4
    m = HipMCMC.run(groups=Metadata.fromFields((2, 0, 1)))
    assert m.groups.tolist() == [0, 0, 2] and m.n_groups == 3
    for bad, exc in (([0, -1], ValueError), ([0.0, 1.0], TypeError), ([[0, 1]], TypeError), ("ab", TypeError), ([0, 4096], ValueError)):
        with pytest.raises(exc):
            HipMCMC.run(groups=bad)
    assert HipMCMC.run(groups=[0, 4095]).n_groups == 4096
    with pytest.raises(RuntimeError, match="first learn"):
        m.group_counts
    # a table shorter than the model raises when the handle is made, before any device call
    from sparkfm_amd import DataSet
    fm = FMModel(6, 2)
    fm._h, fm._dev_fresh = C.c_void_p(1), True                  # (no device: the handle is never used)
    ds = DataSet([0, 1], [0], [1.0], [1.0])
    ds._h = C.c_void_p(2)
    try:
        with pytest.raises(ValueError, match="groups holds 3 ids but the model has num_attribute = 6"):
            m.learn(fm, ds)
    finally:
        fm._h, ds._h = None, None


# ---- the host plan under the sanitizers --------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mcmc_groups") / "host_mcmc_groups_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "host_mcmc_groups_harness.cpp"), os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_host.cpp"), "-o", exe]
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
    """G = 1, a group with no slot, all features in the last group, interleaved ids (stability), a chunk of one slot, no columns, only
    quirk Q1's slot, and 300 random shapes a seed: the chunks cover every trained slot exactly once, sit in group order, never cross
    a group or exceed the chunk size, keep a group's slots ascending; m_a is right."""
    for seed in (20261019, 5):
        assert "checks ok" in harness("check", seed)


def test_the_state_draw_is_the_single_draws_in_the_documented_order(harness):
    """mcmc_draw_state — the one hyper-parameter draw of the flat, the grouped and the relational epoch — for k + 1 = 3 over one group
    with 4 partials, three groups with 0, 1 and 5 partials (the empty group: the draw from the prior) and two parts' 4 partials each as
    one run: alpha, lambda and mu EQUAL mcmc_draw_alpha / mcmc_draw_group called one at a time on sums added sequentially in that order
    with stream id g + (a << 16); the probit form leaves alpha untouched."""
    for seed in (20261020, 7):
        assert "draws ok" in harness("draw", seed)
