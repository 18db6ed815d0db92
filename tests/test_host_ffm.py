"""The field-aware FM's host surface (no GPU): header against binding, the refusals that need no device, loadLibFFMFile, the host dataset
build (tests/host_ffm_harness.cpp, a stand-alone program under ASan and UBSan) against the twin's layout, the twin on the planted task."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ffm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_matches_the_binding():
    from sparkfm_amd import _build, _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip_ffm.h")).read()
    declared = set(re.findall(r"\b(fmhip_ffm_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS_FFM) and len(_ffi.SYMBOLS_FFM) == 15
    L = _ffi.load()
    for name in _ffi.SYMBOLS_FFM:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None, name
    for name, value in (("FIELDS", _ffi.FFM_MAX_FIELDS), ("FACTORS", _ffi.FFM_MAX_FACTORS), ("ROW", _ffi.FFM_MAX_ROW)):
        assert int(re.search(r"#define FMHIP_FFM_MAX_%s (\d+)" % name, hdr).group(1)) == value
    assert "fm_ffm.hip" in _build.HIP_SOURCES and "fmhip_ffm.hip" in _build.HIP_SOURCES and "fm_ffm.h" in _build.HIP_DEPS
    import sparkfm_amd
    assert {"FFM", "FFMDataSet", "FFMModel", "HipFFM"} <= set(sparkfm_amd.__all__)


def test_c_calls_refuse_without_a_device():
    from sparkfm_amd import FFMDataSet, _ffi
    L = _ffi.load()
    err = L.fmhip_last_error
    h = C.c_void_p()
    for call in (lambda: L.fmhip_ffm_model_info(None, None, None, None, None), lambda: L.fmhip_ffm_model_set_params(None, 0.0, None, None),
                 lambda: L.fmhip_ffm_model_get_params(None, None, None, None), lambda: L.fmhip_ffm_model_set_rule(None, 0, 0, 1e-10, 1.0),
                 lambda: L.fmhip_ffm_model_set_linear(None, 1), lambda: L.fmhip_ffm_model_get_accumulators(None, None, None, None),
                 lambda: L.fmhip_ffm_model_set_accumulators(None, 0.0, None, None),
                 lambda: L.fmhip_ffm_dataset_info(None, None, None, None, None, None, None, None), lambda: L.fmhip_ffm_predict(None, None, None),
                 lambda: L.fmhip_ffm_step(None, None, 0, 0.1, 0.0, 0.0, 0.0, None), lambda: L.fmhip_ffm_epoch(None, None, 0.1, 0.0, 0.0, 0.0, None, None)):
        assert call() == -1 and b"handle is NULL" in err()
    assert L.fmhip_ffm_model_destroy(None) == 0 and L.fmhip_ffm_dataset_destroy(None) == 0
    assert L.fmhip_ffm_model_create(0, 10, 2, 4, None, None) == -1 and b"out is NULL" in err()
    for args, code, msg in (((-1, 2, 4), -1, b"num_attribute = -1"), ((10, 0, 4), -1, b"num_fields = 0"), ((10, 65, 4), -5, b"num_fields = 65"),
                            ((10, 2, 0), -1, b"num_factor = 0"), ((10, 2, 17), -5, b"num_factor = 17")):
        assert L.fmhip_ffm_model_create(0, args[0], args[1], args[2], None, C.byref(h)) == code and msg in err(), args
        assert h.value is None

    # the data's limits
    def create(rows, y=None):
        d = FFMDataSet.from_rows(rows, y)          # (host arrays only: no handle is made)
        return L.fmhip_ffm_dataset_create(0, d.size, _ffi.ptr(d.row_ptr), _ffi.ptr(d.col), _ffi.ptr(d.field), _ffi.ptr(d.val), _ffi.ptr(d.y), 0, C.byref(h))
    ok = [(0, 1, 1.0), (1, 2, 1.0)]
    for rows, code, msg in (([ok, [(0, i, 1.0) for i in range(65)]], -5, b"row 1 has 65 entries"), ([ok, [(0, -3, 1.0)]], -1, b"feature id -3"),
                            ([[(64, 1, 1.0)]], -1, b"field id 64"), ([[(-1, 1, 1.0)]], -1, b"field id -1"),
                            ([ok, ok, [(0, 5, 1.0), (1, 5, 2.0)]], -1, b"row 2 holds feature id 5 twice"),
                            ([[(0, 1, float("nan"))]], -1, b"values are finite"), ([[(0, 1, 1e39)]], -1, b"values are finite")):
        assert create(rows) == code and msg in err(), rows
        assert h.value is None
    assert create([ok], y=[float("inf")]) == -1 and b"y[0]" in err()
    arrays = (np.array([0, 2, 1], np.int64), np.array([0, 1], np.int32), np.zeros(2, np.int32), np.zeros(2))
    bad = [_ffi.ptr(x) for x in arrays]
    assert L.fmhip_ffm_dataset_create(0, 2, bad[0], bad[1], bad[2], bad[3], None, 0, C.byref(h)) == -1 and b"row_ptr decreases at row 1" in err()
    assert L.fmhip_ffm_dataset_create(0, 2, None, None, None, None, None, 0, C.byref(h)) == -1 and b"row_ptr is NULL" in err()


def test_libffm_file_round_trip(tmp_path):
    from sparkfm_amd import FMUtils
    path = tmp_path / "five.ffm"
    path.write_text("1 0:3:1 2:7:0.5\n# a comment\n0 1:0:2.5\n\n-1 2:9:1  0:1:-1 1:4:0\n1\n0 63:12:1e-3\n")
    ds = FMUtils.loadLibFFMFile(str(path), batch_rows=2, normalize=False)
    assert ds.size == 5 and ds.y.tolist() == [1, 0, -1, 1, 0] and ds.row_ptr.tolist() == [0, 2, 3, 6, 6, 7]
    assert ds.field.tolist() == [0, 2, 1, 2, 0, 1, 63] and ds.col.tolist() == [3, 7, 0, 9, 1, 4, 12]
    assert ds.val.tolist() == [1, 0.5, 2.5, 1, -1, 0, 1e-3] and ds.dimension == 12 and ds.num_fields == 64 and ds.batch_rows == 2
    unit = FMUtils.loadLibFFMFile(str(path), normalize=True)
    np.testing.assert_allclose(unit.val, [1 / np.sqrt(1.25), 0.5 / np.sqrt(1.25), 1, 1 / np.sqrt(2), -1 / np.sqrt(2), 0, 1], rtol=1e-15)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("ffm")
    exe = str(tmp / "host_ffm_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "host_ffm_harness.cpp"), os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("no sanitizer runtime for g++ in this image")
    assert r.returncode == 0, r.stderr.decode()[-3000:]

    def run(rows, batch_rows, chunk):
        path = tmp / "rows.txt"
        path.write_text("".join(" ".join("%d:%d:%r" % e for e in r) + "\n" for r in rows))
        r = subprocess.run([exe, "layout", str(path), str(batch_rows), str(chunk)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        return r.stdout.decode()
    return run


@pytest.mark.parametrize("batch_rows,chunk", [(0, 256), (7, 4), (1, 1), (1000, 3)])
def test_the_dataset_build_under_the_sanitizers(harness, batch_rows, chunk):
    """Row sort, run heads, transpose and chunk cuts against the twin's layout: rows of 0 .. 64 entries, runs longer than 1, a row of one field."""
    rng = np.random.default_rng(20261126)
    rows = ref.random_rows(rng, 40, 90, 5, [0, 1, 2, 17, 33, 64, 5, 3])
    out = harness(rows, batch_rows, chunk)
    head, body = out.split("\n", 1)
    assert head == "check 0 -1 -1 89 5 64"
    assert body == ref.layout(rows, batch_rows, chunk)
    assert chunk != 3 or re.search(r"chunks [2-9]", body)          # (some column's list is cut)


def test_ffm_beats_fm_on_the_planted_task():
    """The README's two numbers: held-out log-loss of the FFM twin and of the plain-FM twin (every field 0) after 20 epochs of AdaGrad."""
    t = ref.planted()
    _, ffm_train, ffm_test = ref.run_planted(t)
    _, fm_train, fm_test = ref.run_planted(t, fm=True)
    print("FFM: train %.4f test %.4f; FM: train %.4f test %.4f" % (ffm_train, ffm_test, fm_train, fm_test))
    assert ffm_test < fm_test
