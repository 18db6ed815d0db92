"""CPU-only checks of the ranking-metrics surface (include/fmhip_metrics.h): the binding's symbol list against the header and the
library, the header as strict C99, the refusals that need no GPU, the build list — and the numpy twin the GPU tests compare
against (auc_ref.py), itself checked against an O(n^2) pair count."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from auc_ref import FIELDS, auc_brute, auc_ref, same, score_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_metrics_symbols_header_and_library():
    """_ffi.SYMBOLS_METRICS == what include/fmhip_metrics.h declares, all exported by the library, disjoint from the other lists
    and absent from the other headers; the header includes the product header only; the binding's struct is the header's."""
    from sparkfm_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_metrics.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_ffi.SYMBOLS_METRICS) == {"fmhip_auc_scores", "fmhip_auc"}
    assert not declared & set(_ffi.SYMBOLS + _ffi.SYMBOLS_EXPERIMENTAL + _ffi.SYMBOLS_TOPK + _ffi.SYMBOLS_PAIRING)
    assert '#include "fmhip.h"' in code and "fmhip_experimental" not in code
    L = _ffi.load()
    for name in declared:
        assert hasattr(L, name) and getattr(L, name).restype is C.c_int, name
    for other in ("fmhip.h", "fmhip_experimental.h", "fmhip_topk.h", "fmhip_pairing.h"):
        assert "fmhip_auc" not in open(os.path.join(ROOT, "include", other)).read(), other
    # the struct's fields, in the header's order
    body = re.search(r"typedef struct fmhip_auc_result \{(.*?)\} fmhip_auc_result;", code, re.S).group(1)
    names = [n.strip() for decl in re.findall(r"(?:int32_t|uint64_t|int64_t|double)\s+([^;]+);", body) for n in decl.split(",")]
    assert names == [n for n, _ in _ffi.AucResult._fields_]
    assert C.sizeof(_ffi.AucResult) == 72 and _ffi.AucResult().struct_size == 72


def test_metrics_header_is_plain_c(tmp_path):
    src = tmp_path / "t.c"
    src.write_text('#include "fmhip_metrics.h"\n'
                   "int main(void) {\n"
                   "    fmhip_auc_result r;\n"
                   "    r.struct_size = (int32_t)sizeof r;\n"
                   "    return r.struct_size == 72 && FMHIP_VERSION == 500 && fmhip_auc_scores(0, 0, 0, 0, 0, &r) == FMHIP_OK && r.pairs == 0 ? 0 : 1;\n"
                   "}\n")
    from sparkfm_amd import _build
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-L" + _build.LIBDIR, "-lfmhip", "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", str(tmp_path / "t")])
    subprocess.check_call([str(tmp_path / "t")])


def test_auc_kernels_are_built_into_the_library():
    from sparkfm_amd import _build
    assert "fm_auc.hip" in _build.HIP_SOURCES and {"fm_auc.h", "fm_score_key.h"} <= set(_build.HIP_DEPS)
    csrc = os.path.join(ROOT, "sparkfm_amd", "csrc")
    src = re.sub(r"//[^\n]*", "", open(os.path.join(csrc, "fm_auc.hip")).read())      # the code, not its comments
    assert "radix_sort_keys" in src and "atomic" not in src.lower() and not re.search(r"\basm\b", src)
    # one key function, shared: the AUC kernels and top-K rank by the same rule
    for name in ("fm_auc.hip", "fm_topk.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert '#include "fm_score_key.h"' in text and not re.search(r"uint32_t\s+score_key\s*\(", text), name


def test_auc_argument_validation_without_a_gpu():
    """The refusals decided before any handle or device is touched, by status and message; n == 0 is answered on the host."""
    from sparkfm_amd import _ffi, metrics
    L = _ffi.load()
    one = np.zeros(1, np.float32)
    res = _ffi.AucResult()
    assert L.fmhip_auc_scores(0, 1, _ffi.ptr(one), _ffi.ptr(one), None, None) == -1
    assert b"out is NULL" in L.fmhip_last_error()
    assert L.fmhip_auc(None, None, None, None, None) == -1
    assert b"out is NULL" in L.fmhip_last_error()
    bad = _ffi.AucResult()
    bad.struct_size = 64
    assert L.fmhip_auc_scores(0, 1, _ffi.ptr(one), _ffi.ptr(one), None, C.byref(bad)) == -1
    assert b"struct_size" in L.fmhip_last_error()
    assert L.fmhip_auc(None, None, None, C.byref(bad), None) == -1
    assert b"struct_size" in L.fmhip_last_error()
    assert L.fmhip_auc_scores(0, 2 ** 31, _ffi.ptr(one), _ffi.ptr(one), None, C.byref(res)) == -5          # FMHIP_ERR_UNSUPPORTED
    assert b"2^31" in L.fmhip_last_error()
    assert L.fmhip_auc_scores(0, -1, _ffi.ptr(one), _ffi.ptr(one), None, C.byref(res)) == -1
    assert L.fmhip_auc_scores(0, 1, None, _ffi.ptr(one), None, C.byref(res)) == -1
    assert b"NULL" in L.fmhip_last_error()
    assert L.fmhip_auc(None, None, None, C.byref(res), None) == -1
    assert b"NULL" in L.fmhip_last_error()
    # a negative group id names its row
    s, y, g = np.zeros(5, np.float32), np.ones(5, np.float32), np.array([4, 0, 2 ** 31 - 1, -7, 1], np.int32)
    assert L.fmhip_auc_scores(0, 5, _ffi.ptr(s), _ffi.ptr(y), _ffi.ptr(g), C.byref(res)) == -1
    assert b"row 3" in L.fmhip_last_error() and b"-7" in L.fmhip_last_error()
    with pytest.raises(_ffi.FmhipError, match="row 3"):
        metrics.auc(s, y, g)
    # n == 0: OK, zero counts, NaN ratios
    r = metrics.auc([], [])
    assert all(r[k] == 0 for k in FIELDS) and math.isnan(r["auc"]) and math.isnan(r["gauc"])
    assert metrics.auc([], [], groups=np.zeros(0, np.int32)) .keys() == r.keys()
    # the Python mirror's own refusals
    with pytest.raises(ValueError, match="differ in length"):
        metrics.auc([1.0, 2.0], [1.0])
    with pytest.raises(ValueError, match="one id per row"):
        metrics.auc([1.0, 2.0], [1.0, 0.0], groups=[1])
    with pytest.raises(ValueError, match="integers"):
        metrics.auc([1.0, 2.0], [1.0, 0.0], groups=[0.5, 1.0])
    with pytest.raises(ValueError, match="2\\^31"):
        metrics.auc([1.0, 2.0], [1.0, 0.0], groups=[0, 2 ** 31])


def test_score_keys_order():
    vals = np.array([np.nan, -np.inf, -3.0, -1e-45, -0.0, 0.0, 1e-45, 0.25, np.inf], np.float32)
    k = score_keys(vals).astype(np.int64)
    assert k[0] == 0 and k[4] == k[5] and (np.diff(np.delete(k, 4)) > 0).all()
    assert score_keys(np.array([np.nan, -np.nan], np.float32)).tolist() == [0, 0]


VALUES = np.array([-np.inf, -1.5, -0.0, 0.0, 0.25, 3.0, np.inf, np.nan], np.float32)


@pytest.mark.parametrize("grouped", [False, True])
def test_twin_agrees_with_the_pair_count(grouped):
    """150 random cases of up to 40 rows per variant (300 in all), scores from {-Inf, -1.5, -0, +0, 0.25, 3, +Inf, NaN}: every
    integer field, auc and gauc of the twin equal the brute-force count's (both sum gauc group by group in the same order)."""
    rng = np.random.default_rng(7 + grouped)
    for case in range(150):
        n = int(rng.integers(0, 41))
        s = VALUES[rng.integers(0, len(VALUES), n)]
        y = rng.choice(np.array([-1.0, 0.0, 1.0], np.float32), n)
        g = rng.choice(np.array([0, 3, 17, 2 ** 31 - 1]), n) if grouped else None
        a, b = auc_ref(s, y, g), auc_brute(s, y, g)
        for f in FIELDS:
            assert a[f] == b[f], (case, f, a, b)
        assert same(a["auc"], b["auc"]) and same(a["gauc"], b["gauc"]), (case, a, b)
        if not grouped:
            assert same(a["gauc"], a["auc"]) and a["groups"] == min(n, 1)


def test_twin_on_cases_worked_by_hand():
    # one positive above, one tied with, one below a negative: 2U = 2 + 1 + 0 over 3 pairs
    r = auc_ref([2.0, 1.0, 0.5, 1.0], [1, 1, 1, 0])
    assert (r["u2"], r["pairs"], r["positives"], r["negatives"], r["auc"]) == (3, 3, 3, 1, 0.5)
    # NaN ranks below -Inf: the NaN positive loses to the -Inf negative; two NaNs tie
    r = auc_ref([np.nan, -np.inf, np.nan], [1, 0, 0])
    assert (r["u2"], r["pairs"]) == (1, 2)
    # two groups, the second with one class: only the first counts
    r = auc_ref([1.0, 0.0, 5.0, 6.0], [1, 0, 1, 1], [9, 9, 2, 2])
    assert (r["u2"], r["pairs"], r["groups"], r["groups_scored"], r["auc"], r["gauc"]) == (2, 1, 2, 1, 1.0, 1.0)
