"""CPU-only checks of the ranking-evaluation surface (include/fmhip_ranking.h): the binding's symbol list against the header and
the library, the header as strict C99, fmhip_rank_metrics against a known answer and against the numpy restatement
(tests/rank_ref.py), its refusals, and the same arithmetic in a stand-alone program under AddressSanitizer and UBSan."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from rank_ref import FIELDS, rank_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The restatement and the library sum the same terms in the same order; they may differ in log2 and in whether a quotient is
# formed before or after a sum: a few ulp (2^-53) per term, at most 200 contexts x 5 terms per sum.  1e-13 covers 1000 ulp.
RTOL = 1e-13


def known_answer():
    """k = 3: contexts with ranks {0, 3}, {5} and {} (skipped)"""
    l3 = math.log2(3.0)
    want = dict(k=3, contexts=2, skipped=1, relevant=3, hit_rate=1 / 2, recall=1 / 4, precision=1 / 6, ndcg=(1 / (1 + 1 / l3)) / 2,
                mrr=(1 + 1 / 6) / 2, map=(3 / 4 + 1 / 6) / 2)
    return [[3, 0], [5], []], 3, want


def random_rank_sets(n_sets=200, seed=11):
    """200 random rank sets: 0-200 contexts each, every context's |R| in 0-5, ranks below 2000, distinct within a context"""
    rng = np.random.default_rng(seed)
    sets = []
    for i in range(n_sets):
        n = int(rng.integers(0, 201)) if i else 0
        sets.append([rng.choice(2000 if i % 3 else 12, int(rng.integers(0, 6)), replace=False) for _ in range(n)])
    return sets


def close(got, want, rtol):
    for f in ("k", "contexts", "skipped", "relevant"):
        assert got[f] == want[f], (f, got, want)
    for f in FIELDS:
        assert abs(got[f] - want[f]) <= rtol * abs(want[f]), (f, got[f], want[f])


def test_ranking_symbols_header_and_library():
    """_ffi.SYMBOLS_RANKING == what include/fmhip_ranking.h declares == {fmhip_rank, fmhip_rank_metrics}, disjoint from the other
    five lists, exported by the library and absent from the other headers; FMHIP_VERSION stays 500; the binding's struct is the
    header's, field for field."""
    from sparkfm_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_ranking.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_ffi.SYMBOLS_RANKING) == {"fmhip_rank", "fmhip_rank_metrics"}
    others = _ffi.SYMBOLS + _ffi.SYMBOLS_EXPERIMENTAL + _ffi.SYMBOLS_TOPK + _ffi.SYMBOLS_PAIRING + _ffi.SYMBOLS_METRICS
    assert not declared & set(others)
    assert '#include "fmhip_topk.h"' in code and "fmhip_experimental" not in code
    L = _ffi.load()
    assert L.fmhip_version() == 500
    for name in declared:
        assert hasattr(L, name) and getattr(L, name).restype is C.c_int, name
    for other in ("fmhip.h", "fmhip_experimental.h", "fmhip_topk.h", "fmhip_pairing.h", "fmhip_metrics.h"):
        assert not re.search(r"\bfmhip_rank(_metrics\w*)?\b", open(os.path.join(ROOT, "include", other)).read()), other
    body = re.search(r"typedef struct fmhip_rank_metrics \{(.*?)\} fmhip_rank_metrics_t;", code, re.S).group(1)
    names = [n.strip() for decl in re.findall(r"(?:int32_t|int64_t|double)\s+([^;]+);", body) for n in decl.split(",")]
    assert names == [n for n, _ in _ffi.RankMetrics._fields_]
    assert C.sizeof(_ffi.RankMetrics) == 80 and _ffi.RankMetrics().struct_size == 80


def test_ranking_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "fmhip_ranking.h"\n'
                   "int main(void) {\n"
                   "    fmhip_rank_metrics_t r;\n"
                   "    const int64_t ptr[2] = {0, 1};\n"
                   "    const int32_t rank[1] = {1};\n"
                   "    r.struct_size = (int32_t)sizeof r;\n"
                   "    return r.struct_size == 80 && FMHIP_VERSION == 500 && FMHIP_TOPK_MAX == 128 &&\n"
                   "           fmhip_rank_metrics(1, ptr, rank, 2, &r) == FMHIP_OK && r.contexts == 1 && r.mrr == 0.5 &&\n"
                   "           fmhip_rank(0, 0, 0, ptr, rank, 0, 0, 0, 0) == FMHIP_ERR_INVALID ? 0 : 1;\n"
                   "}\n")
    from sparkfm_amd import _build
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-L" + _build.LIBDIR, "-lfmhip", "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", str(tmp_path / "t")])
    subprocess.check_call([str(tmp_path / "t")])


def test_rank_kernels_are_built_into_the_library():
    from sparkfm_amd import _build
    assert "fm_rank.hip" in _build.HIP_SOURCES and {"fm_rank.h", "fm_topk.h", "fm_pair_tiles.h", "fm_score_key.h"} <= set(_build.HIP_DEPS)
    assert any(d.endswith("fmhip_ranking.h") for d in _build.HIP_DEPS)
    csrc = os.path.join(ROOT, "sparkfm_amd", "csrc")
    text = open(os.path.join(csrc, "fm_rank.hip")).read()
    # the code, not its comments: the kernel file together with the tile walk it is built on
    src = re.sub(r"//[^\n]*", "", text + open(os.path.join(csrc, "fm_pair_tiles.h")).read())
    assert "__builtin_amdgcn_mfma_f32_16x16x4f32" in src and "atomic" not in src.lower() and not re.search(r"\basm\b", src)
    for kernel in ("k_pair_list", "k_pair_rank", "k_rank_finish"):
        assert kernel in src, kernel
    # one key function, shared with top-K and the AUC kernels
    assert '#include "fm_score_key.h"' in text and not re.search(r"uint32_t\s+score_key\s*\(", text)
    # one tile walk and one score expression, shared with top-K
    assert '#include "fm_pair_tiles.h"' in text
    assert not re.search(r"float\s+(pair_score|key_score)\s*\(|(void|auto)\s+(fetch|stash)\b", text)


def test_rank_metrics_known_answer():
    from sparkfm_amd import metrics
    ranks, k, want = known_answer()
    close(metrics.ranking_metrics(ranks, k), want, 1e-15)
    close(rank_ref(ranks, k), want, 1e-15)
    # nothing to evaluate: every metric is 0
    for empty in ([], [[], []]):
        got = metrics.ranking_metrics(empty, 5)
        assert got["contexts"] == 0 and got["skipped"] == len(empty) and got["relevant"] == 0
        assert all(got[f] == 0.0 for f in FIELDS)
    # offsets that do not start at 0: ranks are read at the offsets themselves
    from sparkfm_amd import _ffi
    res = _ffi.RankMetrics()
    ptr, flat = np.array([2, 4, 5, 5], np.int64), np.array([77, 77, 3, 0, 5], np.int32)
    assert _ffi.load().fmhip_rank_metrics(3, _ffi.ptr(ptr), _ffi.ptr(flat), 3, C.byref(res)) == 0
    close(res.as_dict(), want, 1e-15)


@pytest.mark.parametrize("k", [1, 10, 128, 1000])
def test_rank_metrics_match_the_numpy_restatement(k):
    from sparkfm_amd import metrics
    for i, ranks in enumerate(random_rank_sets()):
        close(metrics.ranking_metrics(ranks, k), rank_ref(ranks, k), RTOL)


def test_ranking_refusals_without_a_gpu():
    from sparkfm_amd import _ffi, metrics
    L = _ffi.load()
    res = _ffi.RankMetrics()
    ptr, flat = np.array([0, 2, 3], np.int64), np.array([4, 1, 0], np.int32)

    def refused(text, *args):
        assert L.fmhip_rank_metrics(*args) == -1, args
        assert text in L.fmhip_last_error().decode(), L.fmhip_last_error()
    assert L.fmhip_rank_metrics(2, _ffi.ptr(ptr), _ffi.ptr(flat), 1, C.byref(res)) == 0
    refused("negative rank", 2, _ffi.ptr(ptr), _ffi.ptr(np.array([4, -1, 0], np.int32)), 1, C.byref(res))
    refused("twice", 2, _ffi.ptr(ptr), _ffi.ptr(np.array([4, 4, 0], np.int32)), 1, C.byref(res))
    refused("context 0", 2, _ffi.ptr(ptr), _ffi.ptr(np.array([4, 4, 0], np.int32)), 1, C.byref(res))
    refused("k = 0", 2, _ffi.ptr(ptr), _ffi.ptr(flat), 0, C.byref(res))
    refused("k = -3", 2, _ffi.ptr(ptr), _ffi.ptr(flat), -3, C.byref(res))
    bad = _ffi.RankMetrics()
    bad.struct_size = 72
    refused("struct_size", 2, _ffi.ptr(ptr), _ffi.ptr(flat), 1, C.byref(bad))
    refused("out is NULL", 2, _ffi.ptr(ptr), _ffi.ptr(flat), 1, None)
    refused("rel_ptr is NULL", 2, None, _ffi.ptr(flat), 1, C.byref(res))
    refused("rank is NULL", 2, _ffi.ptr(ptr), None, 1, C.byref(res))
    refused("decreases", 2, _ffi.ptr(np.array([0, 2, 1], np.int64)), _ffi.ptr(flat), 1, C.byref(res))
    refused("rel_ptr[0] < 0", 2, _ffi.ptr(np.array([-1, 2, 3], np.int64)), _ffi.ptr(flat), 1, C.byref(res))
    refused("negative", -1, _ffi.ptr(ptr), _ffi.ptr(flat), 1, C.byref(res))
    with pytest.raises(_ffi.FmhipError, match="twice"):
        metrics.ranking_metrics([[1, 1]], 3)
    with pytest.raises(_ffi.FmhipError, match="k = 0"):
        metrics.ranking_metrics([[1]], 0)
    # fmhip_rank refuses a NULL handle before it touches a device
    one = np.zeros(2, np.int64)
    assert L.fmhip_rank(None, None, None, _ffi.ptr(one), None, None, None, None, None) == -1
    assert b"NULL" in L.fmhip_last_error()
    # the Python mirror's own refusals
    from sparkfm_amd import DataSet, FMModel
    fm = FMModel(10, 4)
    rows = DataSet(np.array([0, 1], np.int64), np.array([1], np.int32), np.array([1.0]), np.zeros(1), scoring=True)
    with pytest.raises(ValueError, match="relevant must hold one array per context"):
        fm.rankOf(rows, rows, [[0], [0]])
    with pytest.raises(ValueError, match="relevant names a candidate row outside"):
        fm.rankOf(rows, rows, [[1]])
    with pytest.raises(ValueError, match="exclude names a candidate row outside"):
        fm.rankOf(rows, rows, [[0]], exclude=[[-1]])
    with pytest.raises(ValueError, match="both relevant and excluded"):
        fm.rankOf(rows, rows, [[0]], exclude=[[0]])
    with pytest.raises(ValueError, match="k must be"):
        fm.computeRankingMetrics(rows, rows, [[0]], k=0)


def test_rank_metrics_under_the_sanitizers(tmp_path):
    """tests/host_rank_harness.cpp + fmhip_host.cpp built with g++ -fsanitize=address,undefined, run as a subprocess over the known
    answer, the 200 random rank sets at four k, and the two refusals the arithmetic itself decides."""
    exe = str(tmp_path / "host_rank_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "host_rank_harness.cpp"), os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("no sanitizer runtime for g++ in this image")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    ranks, k, want = known_answer()
    cases = [(ranks, k, want), ([[2, -1]], 4, None), ([[1], [7, 3, 7]], 4, None)]
    for k in (1, 10, 128, 1000):
        cases += [(s, k, rank_ref(s, k)) for s in random_rank_sets()]
    path = tmp_path / "cases.txt"
    with open(path, "w") as f:
        for s, k, _ in cases:
            ptr = np.concatenate([[0], np.cumsum([len(r) for r in s])]).astype(np.int64)
            f.write("%d %d\n%s\n%s\n" % (k, len(s), " ".join(map(str, ptr)), " ".join(str(int(x)) for r in s for x in r)))
    r = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"),
                       timeout=600)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    lines = [ln.split() for ln in r.stdout.decode().split("\n") if ln.strip()]
    assert len(lines) == len(cases)
    for (s, k, want), ln in zip(cases, lines):
        if want is None:
            assert int(ln[0]) == len(s) - 1          # the last context is the bad one
            continue
        got = dict(k=k, contexts=int(ln[1]), skipped=int(ln[2]), relevant=int(ln[3]))
        got.update({f: float.fromhex(x) for f, x in zip(FIELDS, ln[4:])})
        assert int(ln[0]) == -1
        close(got, want, 1e-15 if s is ranks else RTOL)
