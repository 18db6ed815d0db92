"""CPU-only checks of the top-K recommendation surface (include/fmhip_topk.h): the pair identity the whole feature rests
on, the binding's third symbol list against the header and the library, argument validation that needs no GPU, the build."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
from topk_ref import field_rows, joined, pair_ref, params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed,B,M,n,k", [(1, 7, 11, 40, 5), (2, 5, 9, 64, 32), (3, 12, 6, 30, 1), (4, 3, 17, 200, 70)])
def test_pair_identity(seed, B, M, n, k):
    """predict(c ++ d) = predict(c) + predict(d) - w0 + sum_f q_f(c) q_f(d) for rows over disjoint id ranges (contexts over
    [0, n/2), candidates over [n/2, n]), empty rows on both sides: oracle.predict of the explicitly joined rows equals the
    right-hand side to 1e-12 relative."""
    w0, w, v = params(seed, n + 1, k, scale=0.3)
    ctx = field_rows(10 + seed, B, [(0, n // 4), (n // 4, n // 2)], empty=(1,), half=False)
    cand = field_rows(20 + seed, M, [(n // 2, 3 * n // 4), (3 * n // 4, n + 1), (n // 2, n + 1)][:2], empty=(0, M - 1), half=False)
    pairs = [(c, d) for c in range(B) for d in range(M)]
    j = joined(ctx, cand, pairs)
    lhs = oracle.predict(w0, w, v, j["row_ptr"], j["col"], j["val"]).reshape(B, M)
    S, tol = pair_ref(w0, w, v, ctx, cand)
    assert (np.abs(lhs - S) <= 1e-12 * (1.0 + np.abs(S))).all(), float(np.abs(lhs - S).max())
    assert (tol > 0).all()
    # an empty context with an empty candidate scores w0
    assert S[1, 0] == pytest.approx(w0, abs=1e-15)


def test_topk_symbols_header_and_library():
    """_ffi.SYMBOLS_TOPK == what include/fmhip_topk.h declares, all exported by the library, disjoint from the other two lists;
    the header includes the product header and the binding's K limit is the header's."""
    from sparkfm_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_topk.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", code))
    assert declared == set(_ffi.SYMBOLS_TOPK) == {"fmhip_topk", "fmhip_pair_scores"}
    assert not declared & (set(_ffi.SYMBOLS) | set(_ffi.SYMBOLS_EXPERIMENTAL))
    assert '#include "fmhip.h"' in code and "fmhip_experimental" not in code
    assert int(re.search(r"#define FMHIP_TOPK_MAX (\d+)", code).group(1)) == _ffi.TOPK_MAX == 128
    L = _ffi.load()
    for name in declared:
        assert hasattr(L, name) and getattr(L, name).restype is C.c_int, name
    for other in ("fmhip.h", "fmhip_experimental.h"):
        assert "fmhip_topk" not in open(os.path.join(ROOT, "include", other)).read()


def test_topk_kernels_are_built_into_the_library():
    from sparkfm_amd import _build
    assert "fm_topk.hip" in _build.HIP_SOURCES and {"fm_topk.h", "fm_pair_tiles.h"} <= set(_build.HIP_DEPS)
    csrc = os.path.join(ROOT, "sparkfm_amd", "csrc")
    text = open(os.path.join(csrc, "fm_topk.hip")).read()
    # the code, not its comments: the kernel file together with the tile walk it is built on
    src = re.sub(r"//[^\n]*", "", text + open(os.path.join(csrc, "fm_pair_tiles.h")).read())
    assert "__builtin_amdgcn_mfma_f32_16x16x4f32" in src and "atomic" not in src.lower() and not re.search(r"\basm\b", src)
    # one tile walk and one score expression, shared with the rank kernels
    assert '#include "fm_pair_tiles.h"' in text
    assert not re.search(r"float\s+(pair_score|key_score)\s*\(|(void|auto)\s+(fetch|stash)\b", text)


def test_topk_header_is_plain_c(tmp_path):
    import subprocess
    src = tmp_path / "t.c"
    src.write_text('#include "fmhip_topk.h"\nint main(void) { return FMHIP_TOPK_MAX == 128 && FMHIP_VERSION == 500 ? 0 : 1; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-o", str(tmp_path / "t")])
    subprocess.check_call([str(tmp_path / "t")])


def test_topk_argument_validation_without_a_gpu():
    """The refusals that are decided before any handle is dereferenced, by status and message; and the Python mirror's own."""
    from sparkfm_amd import _ffi, DataSet, FMModel
    L = _ffi.load()
    idx = np.zeros(4, np.int32)
    out = np.zeros(4)
    assert L.fmhip_topk(None, None, None, 1, None, None, _ffi.ptr(idx), None) == -1
    assert b"NULL" in L.fmhip_last_error()
    assert L.fmhip_pair_scores(None, None, None, 0, 0, _ffi.ptr(out)) == -1
    assert b"NULL" in L.fmhip_last_error()
    fm = FMModel(10, 4)
    rows = DataSet(np.array([0, 1], np.int64), np.array([1], np.int32), np.array([1.0]), np.zeros(1), scoring=True)
    for k in (0, -1, 129):
        with pytest.raises(ValueError, match="k must be"):
            fm.recommend(rows, rows, k)
    with pytest.raises(ValueError, match="one array per context"):
        fm.recommend(rows, rows, 1, exclude=[[0], [0]])
    with pytest.raises(ValueError, match="outside"):
        fm.recommend(rows, rows, 1, exclude=[[1]])
    with pytest.raises(ValueError, match="outside"):
        fm.pairScores(rows, rows, 1, 0)
