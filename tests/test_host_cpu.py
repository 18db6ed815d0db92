"""CPU-only checks of the host side: the C-ABI library loads and exports every symbol the
header declares, argument validation that needs no GPU, the host mirrors of the reference
classes, the synthetic generator, and the build entry point."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    """Both headers against the binding's two symbol lists and the library: include/fmhip.h is the product surface (what
    INTEGRATION.md section 1 maps to a reference interface + the data-parallel step), include/fmhip_experimental.h the
    measurement / experiment surface; no symbol sits in both, the library exports all of them, and the tuning keys are a
    named enum whose values the binding (and the kernels' own enum, by static_assert in fmhip_api.hip) agree with."""
    from sparkfm_amd import _ffi
    hdr = open(os.path.join(ROOT, "include", "fmhip.h")).read()
    exp = open(os.path.join(ROOT, "include", "fmhip_experimental.h")).read()
    declared = set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", hdr))
    declared_exp = set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", exp, flags=re.S)))
    assert declared == set(_ffi.SYMBOLS)
    assert declared_exp == set(_ffi.SYMBOLS_EXPERIMENTAL)
    assert not declared & declared_exp
    # the lab equipment is NOT in the product header
    for name in ("fmhip_tune", "fmhip_comm_emulate", "fmhip_ablation_mask", "fmhip_dataset_band_plan", "fmhip_device_read", "fmhip_profile_begin"):
        assert name not in declared and name in declared_exp, name
    assert len(declared) <= 64
    L = _ffi.load()
    for name in declared | declared_exp:
        assert hasattr(L, name), name
    m = re.search(r"#define FMHIP_VERSION (\d+)", hdr)
    assert L.fmhip_version() == int(m.group(1)) == 500
    m = re.search(r"#define FMHIP_RANGE_LEN (\d+)", hdr)
    assert int(m.group(1)) == _ffi.RANGE_LEN
    keys = dict((k, int(v)) for k, v in re.findall(r"\bFMHIP_TUNE_([A-Z_]+) = (\d+)", exp))
    assert keys.pop("KEY_COUNT") == len(keys) == len(_ffi.TUNE) and keys == _ffi.TUNE


def test_shipped_build_carries_no_ablation():
    """The kernel sources hold timing-only ablation switches (FMHIP_EXP_*: parts of the arithmetic or the traffic compiled out,
    results wrong by construction).  The shipped build must have none set: the flags of sparkfm_amd/_build.py name none, the
    sources refuse to compile with one unless the build declares itself an ablation build, and the library reports a zero mask."""
    from sparkfm_amd import _build, _ffi
    assert not any("FMHIP_EXP" in f or "FMHIP_ABLATION" in f for f in _build.HIPCC_FLAGS)
    assert _ffi.load().fmhip_ablation_mask() == 0
    for name in ("fm_forward.hip", "fm_backward.hip"):
        src = open(os.path.join(ROOT, "sparkfm_amd", "csrc", name)).read()
        assert "!defined(FMHIP_ABLATION_BUILD)" in src and "#error" in src
        for m in set(re.findall(r"FMHIP_EXP_[A-Z0-9_]+", src)):
            assert re.search(r"#define %s 0\b" % m, src), m          # every switch defaults to off


def test_argument_validation_without_a_gpu():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    h = C.c_void_p()
    assert L.fmhip_model_create(0, 10, 4, None, None) == -1
    assert L.fmhip_model_create(0, -1, 4, None, C.byref(h)) == -1
    assert L.fmhip_model_create(0, 10, 0, None, C.byref(h)) == -1
    assert L.fmhip_model_create(0, 10, 10_000, None, C.byref(h)) == -5
    assert b"FMHIP_MAX_FACTORS" in L.fmhip_last_error()
    rp = np.array([0, 2, 1], np.int64)
    assert L.fmhip_dataset_create(0, 2, rp.ctypes.data, None, None, None, 0, C.byref(h)) == -1
    assert b"row_ptr decreases" in L.fmhip_last_error()
    assert L.fmhip_model_destroy(None) == 0 and L.fmhip_dataset_destroy(None) == 0
    assert L.fmhip_predict(None, None, None) == -1


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from sparkfm_amd import _ffi
    monkeypatch.setattr(_ffi, "_lib", None)
    monkeypatch.setattr(_ffi, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(ImportError, match="no CPU fallback"):
        _ffi.load()


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "sparkfm_amd")
    for dp, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".hip", ".h", ".c", ".cpp")):
                src = open(os.path.join(dp, fn)).read()
                assert not re.search(r"^\s*(import|from)\s+oracle\b", src, re.M), fn
                assert "fm_oracle" not in src, fn


def test_dataset_host_mirror():
    from sparkfm_amd import DataSet
    rows = [(1.0, ([0, 2, 3], [1.0, 2.0, 0.5])), (-1.0, ([1, 2], [1.0, 1.0])), (2.0, ([0], [3.0])), (0.5, ([], []))]
    ds = DataSet.apply("toy", rows)
    assert ds.size == 4 and ds.dimension == 3 and ds.nnz == 6 and not ds.isEmpty
    assert list(ds.row_ptr) == [0, 3, 5, 6, 6]
    back = list(ds.rows())
    assert back[1][0] == -1.0 and list(back[1][1][0]) == [1, 2]
    assert DataSet.from_rows([]).isEmpty and DataSet.from_rows([]).dimension == 0
    with pytest.raises(ValueError):
        DataSet([0, 2], [0], [1.0], [1.0])


def test_model_host_layout_matches_breeze_column_major():
    from sparkfm_amd import FMModel
    fm = FMModel(5, 3, seed=1)
    assert fm.w.shape == (6,) and fm.v.shape == (3, 6) and fm.w0 == 0.0
    assert (fm.reg0, fm.regw, fm.regv) == (0.0, 0.0, 10.0)          # S/fm/FMModel.scala:29-31
    flat = fm.v.reshape(-1, order="F")
    assert flat[1 + 4 * 3] == fm.v[1, 4]                             # element (f, i) at f + i*k
    assert abs(fm.v.std() - 0.01) < 0.01
    fm2 = FMModel(5, 3, seed=1)
    np.testing.assert_array_equal(fm.v, fm2.v)


def test_batch_order_is_reproducible():
    from sparkfm_amd import HipSGD
    a, b = HipSGD(shuffle_seed=3), HipSGD(shuffle_seed=3)
    assert list(a.batch_order(8)) == list(b.batch_order(8))
    assert sorted(a.batch_order(8)) == list(range(8))
    a._epoch = 1
    assert list(a.batch_order(8)) != list(b.batch_order(8))
    assert HipSGD().batch_order(8) is None


def test_fit_loop_order(monkeypatch):
    """computeRMSE is called BEFORE each learn (S/fm/impl/FactorizationMachines.scala:42-46)."""
    import sparkfm_amd
    from sparkfm_amd import fm as fm_mod
    calls = []

    class FakeModel:
        def __init__(self, n, k, **kw):
            calls.append(("new", n, k))

        def computeRMSE(self, ds):
            calls.append("rmse")
            return 1.0

    class FakeDS:
        dimension, device, name = 7, 0, "x"

        def cache(self):
            calls.append("cache")
            return self

        def unpersist(self):
            calls.append("unpersist")

    class Learner(sparkfm_amd.FMLearn):
        def learn(self, fm, ds):
            calls.append("learn")
            return fm

    monkeypatch.setattr(fm_mod, "FMModel", FakeModel)
    sparkfm_amd.FM(FakeDS(), 4, maxIteration=2).learnWith(Learner())
    assert calls == ["cache", ("new", 7, 4), "rmse", "learn", "rmse", "learn", "unpersist"]


def test_synth_is_seeded_and_shardable():
    from sparkfm_amd import synth
    a = synth.make_zipf(5, 300, 1000, 5, 15, 1.05)
    b = synth.make_zipf(5, 300, 1000, 5, 15, 1.05)
    for key in ("row_ptr", "col", "val", "y"):
        np.testing.assert_array_equal(a[key], b[key])
    part = synth.make_zipf(5, 100, 1000, 5, 15, 1.05, row_begin=100)
    lo, hi = a["row_ptr"][100], a["row_ptr"][200]
    np.testing.assert_array_equal(part["col"], a["col"][lo:hi])
    np.testing.assert_array_equal(part["y"], a["y"][100:200])
    nn = np.diff(a["row_ptr"])
    assert nn.min() >= 5 and nn.max() <= 15
    for r in range(300):                                            # distinct ids inside a row
        s = a["col"][a["row_ptr"][r]:a["row_ptr"][r + 1]]
        assert len(set(s.tolist())) == len(s)
    assert a["col"].max() < 1000 and (a["val"] > 0).all() and (a["val"] <= 1).all()
    assert (a["col"] == 0).mean() > (a["col"] == 500).mean()       # Zipf: low ids are hot


def test_shard_rows_partition():
    from sparkfm_amd.distributed import shard_rows
    cuts = [shard_rows(1003, r, 8) for r in range(8)]
    assert cuts[0][0] == 0 and cuts[-1][1] == 1003
    assert all(cuts[i][1] == cuts[i + 1][0] for i in range(7))


def test_libfm_io_follows_the_reference(tmp_path):
    """S/fm/FMUtils.scala:23-69 incl. quirk Q9 (the saver writes i+1, the loader keeps indices as written)."""
    from sparkfm_amd import DataSet, FMUtils
    src = tmp_path / "in.libfm"
    src.write_text("# comment\n\n  1 0:1 3:0.5  7:2.25\n-1.5 2:1\n0\n3 5:0.1234 1:1e-3\n")
    ds = FMUtils.loadLibFMFile(str(src))
    assert ds.size == 4 and ds.dimension == 7 and list(ds.row_ptr) == [0, 3, 4, 4, 6]
    assert list(ds.col) == [0, 3, 7, 2, 5, 1] and list(ds.y) == [1.0, -1.5, 0.0, 3.0]   # stored order kept
    out = tmp_path / "out.libfm"
    FMUtils.saveAsLibFMFile(ds, str(out))
    assert out.read_text().splitlines() == ["1 1:1 4:.5 8:2.25", "-1.5 3:1", "0", "3 6:.123 2:.001"]
    FMUtils.saveAsLibFMFile(ds, str(out), index_offset=0)
    back = FMUtils.loadLibFMFile(str(out))
    assert list(back.col) == list(ds.col) and list(back.row_ptr) == list(ds.row_ptr)
    for v, s in [(1.0, "1"), (-2.0, "-2"), (0.5, ".5"), (-0.25, "-.25"), (0.0005, "0"), (0.0015, ".002"),
                 (0.0025, ".002"), (12.3456, "12.346"), (1e-9, "0")]:
        assert FMUtils.minimizeString(v) == s, (v, FMUtils.minimizeString(v))
    with pytest.raises(ValueError):
        FMUtils.loadLibFMFile(str(src), numFeatures=3)


def test_split_by_random():
    from sparkfm_amd import DataCollection, DataSet
    rng = np.random.default_rng(0)
    rows = [(float(i), (rng.choice(50, 3, replace=False), rng.random(3))) for i in range(2000)]
    ds = DataSet.from_rows(rows)
    c = DataCollection.splitByRandom(ds, 0.8, 0.2, seed=4)
    assert c.trainingSet.size + c.testSet.size == 2000 and c.validationSet.size == 0
    assert 0.75 < c.trainingSet.size / 2000 < 0.85
    assert sorted(np.concatenate([c.trainingSet.y, c.testSet.y]).tolist()) == [float(i) for i in range(2000)]
    r0 = int(c.testSet.y[0])
    np.testing.assert_array_equal(c.testSet.col[:3], ds.col[3 * r0:3 * r0 + 3])
    assert c.dimension == max(c.trainingSet.dimension, c.testSet.dimension)
    c3 = DataCollection.splitByRandom(ds, 0.6, 0.2, 0.2, seed=4)
    assert c3.validationSet.size > 0 and c3.trainingSet.size + c3.testSet.size + c3.validationSet.size == 2000
    with pytest.raises(Exception, match="required"):
        DataCollection.splitByRandom(ds, 0.0, 1.0)


def test_plain_c_consumer_of_the_header(tmp_path):
    """include/fmhip.h is C, not just C++, and is ENOUGH: tests/c_abi_smoke.c includes the slim product header alone,
    compiles as strict C99, links against libfmhip.so and exercises the entry points that need no GPU;
    tests/c_abi_experimental_smoke.c does the same for include/fmhip_experimental.h."""
    import subprocess
    from sparkfm_amd import _build
    for name in ("c_abi_smoke", "c_abi_experimental_smoke"):
        src = open(os.path.join(ROOT, "tests", name + ".c")).read()
        assert ('#include "fmhip_experimental.h"' in src) == (name != "c_abi_smoke") and ('#include "fmhip.h"' in src) == (name == "c_abi_smoke")
        exe = str(tmp_path / name)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", name + ".c"), "-L" + _build.LIBDIR, "-lfmhip",
                               "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
        out = subprocess.check_output([exe]).decode()
        assert name + " ok" in out


def test_jni_shim_compiles_and_marshals_like_the_c_abi(tmp_path):
    """jvm/fmhip_jni.c has never met a JDK here.  Compiled against a stand-in jni.h (tests/jni_stub: the JNI specification's
    signatures for the entries the shim uses) with warnings as errors, every call into include/fmhip.h is checked for argument
    count and type; tests/jni_harness.c then drives the natives that are host arithmetic through an in-memory JNIEnv that
    hands out COPIES of the arrays and poisons them on release (the least convenient VM the specification allows) and
    compares each with the same call through the C ABI.  (The GPU natives: test_gpu_configs.py.)"""
    import subprocess
    from helpers import build_jni_harness
    out = subprocess.check_output([build_jni_harness(tmp_path), "host"]).decode()
    assert "jni_harness host:" in out and "checks ok" in out
    # the same under AddressSanitizer + UBSan (the shim's pin / release bookkeeping is exactly what they watch)
    try:
        exe = build_jni_harness(tmp_path, sanitize=True)
    except subprocess.CalledProcessError:
        pytest.skip("no sanitizer runtime for gcc in this image")
    r = subprocess.run([exe, "host"], env=dict(os.environ, ASAN_OPTIONS="detect_leaks=0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and b"checks ok" in r.stdout, r.stderr.decode()[-3000:]


def test_nnz_balanced_shards():
    """fmhip_shard_rows: contiguous, covering, balanced by stored nonzeros — on skewed rows a
    row-count split would be badly off."""
    from sparkfm_amd.distributed import shard_rows
    rng = np.random.default_rng(5)
    lens = np.where(rng.random(20000) < 0.01, rng.integers(500, 3000, 20000), rng.integers(0, 10, 20000))
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    for world in (1, 2, 3, 8):
        sh = [shard_rows(rp, r, world) for r in range(world)]
        assert sh[0][0] == 0 and sh[-1][1] == 20000
        assert all(sh[i][1] == sh[i + 1][0] for i in range(world - 1))
        nnz = np.array([rp[b] - rp[a] for a, b in sh], np.float64)
        assert nnz.max() - nnz.min() <= 2 * lens.max()                  # within a row or two of perfect balance
    assert shard_rows(100, 1, 4) == (25, 50)                            # a bare row count: balanced by rows
    assert [shard_rows(np.zeros(7, np.int64), r, 3) for r in range(3)] == [(0, 2), (2, 4), (4, 6)]


def test_bench_without_a_launcher_fails_cleanly_when_ranks_cannot_start():
    """`python bench.py --gpus 2` with WORLD_SIZE unset spawns the ranks itself; in this container they die at
    once (no GPU) and the parent must report that — not hang waiting on a collective."""
    import subprocess
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=180)
    import torch
    if not torch.cuda.is_available():
        assert p.returncode != 0 and p.stdout.strip() == b""


def test_committed_bench_line_keeps_the_contract():
    """The bench line committed under profiles/ (a real MI355X run of `python bench.py`) carries every key of the
    driver's contract plus the roofline / cpu_baseline objects; the roofline is an HBM-side fraction — counter bytes per
    launch / launch time / 8 TB/s, measured in that run, <= 1 — with the algorithmic figure flagged beside it."""
    import json
    d = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_c3_n1.json")))
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in d, key
    assert d["unit"] == "nnz/s" and d["dtype"] == "f32" and d["data"] == "synthetic" and d["higher_is_better"] is True
    assert d["vs_baseline"] is None and "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] == pytest.approx(d["config"]["nnz_per_gpu"] / d["config"]["batches_per_gpu"] / (d["ms_per_step"] * 1e-3), rel=0.02)
    r = d["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r, key
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and r["traffic_measured_in_this_run"] is True
    assert r["achieved"] == pytest.approx(r["traffic"] / (r["avg_launch_ms"] * 1e-3) / 1e9) and r["frac"] == pytest.approx(r["achieved"] / r["peak"])
    assert 0 < r["frac"] <= 1.0 and 0 < r["step"]["frac"] <= 1.0 and 0 < r["frac_of_ceiling"] <= 1.0 and r["algorithmic_frac"] > 0
    assert 0 < d["step_roofline"]["frac"] <= 1.0
    for k_ in d["kernels"].values():
        if "frac_of_ceiling" in k_:
            assert 0 < k_["frac_of_ceiling"] <= 1.0
        if "traffic_frac_of_8TBps" in k_:
            assert 0 < k_["traffic_frac_of_8TBps"] <= 1.0
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] >= 1 and c["unit"] == "nnz/s" and c["sample"]
    x = d["extra"]
    assert d["sustained"]["seconds"] >= 2.0 and x["hbm_resident"]["frac_of_8TBps"] <= 1.0 and x["hbm_resident"]["distinct_batches"] >= 24
    # round 5: the record says what bounds the step, carries the HBM-resident leg's fraction at the top level, and is the run's
    # LAST line (every leg ran: nothing skipped); the driver's short run (--steps 20 --warmup 5) reproduces it within 1 %
    assert d["record"]["final"] is True and not d["legs"]["skipped"] and d["legs"]["elapsed_s"] < d["legs"]["time_budget_s"]
    assert r["algorithmic_frac"] > 1.0 and r["algorithmic_label"].startswith("model not a bound")
    assert 2.0e8 < r["compulsory_hbm_bytes_per_step"] < 3.5e8 and r["hbm_floor_ms"] == pytest.approx(r["compulsory_hbm_bytes_per_step"] / 8e12 * 1e3)
    assert 0 < r["hbm_floor_share_of_step"] < 0.25 and 0 < r["step_ceiling_frac"] <= 1.0
    assert r["hbm_resident"]["frac"] == pytest.approx(x["hbm_resident"]["frac_of_8TBps"]) and 0.4 < r["hbm_resident"]["frac"] <= 1.0
    short = json.load(open(os.path.join(ROOT, "profiles", "r05_bench_c3_driver_flags.json")))
    assert short["steps"] == 20 and short["warmup"] == 5 and short["value"] == pytest.approx(d["value"], rel=0.01)
    assert x["hbm_resident"]["ids_as_hashed"]["value"] > 0 and x["c4_one_gpu"]["value"] > 0 and len(x["als_long_columns"]) == 3
    assert d["config"]["backward_band_plan"]["band_affine"] > 0
    # round 4: the hit rates the ceilings are blended with come from a counter pass of the run itself; every kernel of the
    # HBM-resident leg stays under its ceiling (round 3's forward read 1.003); relabelling runs on the GPU; the ALS field leg
    for name in ("forward", "backward"):
        assert d["kernels"][name]["ceiling"]["l2_hit_source"].startswith("rocprofv3")
    for k_ in x["hbm_resident"]["kernels"].values():
        assert k_.get("frac_of_ceiling") is None or 0 < k_["frac_of_ceiling"] <= 1.0
    assert x["hbm_resident"]["setup_s"]["relabel"] < 1.0
    assert x["als_fields"]["levels"] == 2 and x["als_fields"]["cpu_over_gpu"] > 1 and x["als_fields"]["max_abs_parameter_difference_after_one_epoch"] < 1e-8
    # the N > 1 record of the eight thread-ranks on one GPU (a rehearsal, not a measurement): complete
    d8 = json.load(open(os.path.join(ROOT, "profiles", "r04_dp8_c5_touched_threads.json")))
    assert d8["n_gpus"] == 8 and d8["exchange"]["nranks"] == 8 and d8["exchange"]["mode"] == "touched"
    assert 1.5e6 < d8["exchange"]["mean_union_rows"] < 2.5e6 and d8["train"]["nonfinite"] == 0


def test_feature_order_utilities_are_host_arithmetic():
    """fmhip_feature_counts / fmhip_rank_from_counts / fmhip_relabel_columns against numpy (no GPU involved):
    descending count, ties by ascending id; accumulation over partitions; in-place relabelling; bad ids refused."""
    from sparkfm_amd import FeatureOrder, _ffi
    rng = np.random.Generator(np.random.PCG64(11))
    for n1, nnz in ((7, 0), (50, 400), (5000, 300_000), ((1 << 23) + 3, 200_000)):
        col = (rng.zipf(1.3, nnz) % n1).astype(np.int32)
        perm = rng.permutation(n1).astype(np.int32)
        col = perm[col]                                   # frequent ids anywhere in the id space
        cnt = FeatureOrder.counts(col[: nnz // 2], n1)
        FeatureOrder.counts(col[nnz // 2:], n1, into=cnt)  # two partitions into one table
        assert np.array_equal(cnt, np.bincount(col, minlength=n1))
        order = FeatureOrder.from_counts(cnt)
        want = np.lexsort((np.arange(n1), -cnt)).astype(np.int32)      # by count descending, then id ascending
        assert np.array_equal(order.by_rank, want)
        assert np.array_equal(order.rank[order.by_rank], np.arange(n1))
        new = order.relabel(col)
        assert np.array_equal(order.by_rank[new], col)
        if nnz:
            c2 = np.bincount(new, minlength=n1)
            assert np.all(np.diff(c2) <= 0)               # counts now fall with the id
        buf = col.copy()
        order.relabel(buf, out=buf)                       # `out` may be `col`
        assert np.array_equal(buf, new)
        w = rng.normal(size=n1) if n1 < 10_000 else np.zeros(n1)
        v = rng.normal(size=(3, n1)) if n1 < 10_000 else np.zeros((3, n1))
        wi, vi = order.to_internal(w, v)
        assert np.array_equal(wi[order.rank], w) and np.array_equal(vi[:, order.rank], v)
        wb, vb = order.to_caller(wi, vi)
        assert np.array_equal(wb, w) and np.array_equal(vb, v)
    bad = np.array([0, 3, 9], np.int32)
    L = _ffi.load()
    cnt = np.zeros(5, np.int64)
    assert L.fmhip_feature_counts(3, bad.ctypes.data, 5, cnt.ctypes.data) == -1
    assert b"outside" in L.fmhip_last_error()
    assert L.fmhip_relabel_columns(3, bad.ctypes.data, 5, np.arange(5, dtype=np.int32).ctypes.data, bad.ctypes.data) == -1
    ident = FeatureOrder.identity(6)
    assert np.array_equal(ident.relabel(np.array([5, 0, 2], np.int32)), [5, 0, 2])


def test_bench_steps_and_dump_sample():
    """bench.py's arguments: --steps is the count of timed steps (at least one: ms_per_step divides by it).  --dump-outputs
    writes every parameter row of a model that fits its 64 MB, and otherwise the same sample of ids in every run — the lowest
    ids and a seeded draw from the rest, sorted and distinct — within it."""
    sys.path.insert(0, ROOT)
    import bench
    a = bench.parse_args(["--steps", "7", "--warmup", "0", "--dump-outputs", "out"])
    assert a.steps == 7 and a.warmup == 0 and a.dump_outputs == "out" and bench.parse_args([]).dump_outputs == ""
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse_args(bad)
    assert np.array_equal(bench.dump_ids(100_000, 32), np.arange(100_000))            # C3: the whole model
    for n1, k in ((1_000_000, 32), (1 << 25, 64)):                                     # C4, C5: a sample
        ids = bench.dump_ids(n1, k)
        assert np.array_equal(ids, bench.dump_ids(n1, k)) and ids.dtype == np.int32
        assert (np.diff(ids) > 0).all() and ids[0] == 0 and ids[-1] < n1 and ids[len(ids) // 2 - 1] == len(ids) // 2 - 1
        assert len(ids) * (k + 2) * 8 <= 60 << 20 and len(ids) > 100_000


def test_bench_full_is_opt_in():
    """A plain bench.py run prints the headline alone; the legs, the kernel pass and the roofline run only with --full."""
    sys.path.insert(0, ROOT)
    import bench
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full", "--time-budget", "100"]).full is True


def test_bench_roofline_helpers():
    """bench.py's byte accounting and ceilings (pure arithmetic): ceilings stay between the Infinity-Cache and the L2
    gather rates, grow with the L2 hit rate, fall back to the HBM gather rate only when nothing is known about a table
    beyond the Infinity Cache; the backward's requested bytes follow the entries left in the transposes; the committed
    PMC entries of the HBM-resident leg are found for the C5 configuration."""
    sys.path.insert(0, ROOT)
    import bench
    lo, hi = bench.CEIL["mall_gather"], bench.CEIL["l2_gather"]
    prev = 0.0
    for h in (0.0, 0.3, 0.74, 1.0):
        name, c, got = bench.gather_ceiling(32 << 20, h)
        assert lo - 1 <= c <= hi + 1 and c > prev and got == h
        prev = c
    assert bench.gather_ceiling(1 << 20)[1] == pytest.approx(hi)                     # fits one XCD's L2
    assert bench.gather_ceiling(9 << 30)[:2] == ("hbm_gather", bench.CEIL["hbm_gather"])
    name, c, _ = bench.gather_ceiling(9 << 30, 0.68)
    assert "upper bound" in name and lo < c < hi
    base = bench.requested_bytes(32, 250_000, 10_000_000, 8_000_000, 90_000, True, 90_000, True, 100_001, False)
    paged = bench.requested_bytes(32, 250_000, 10_000_000, 8_000_000, 90_000, True, 90_000, True, 100_001, False, 6_600_000, 4)
    assert paged["forward"] == base["forward"] and paged["apply"] == base["apply"]
    assert base["backward"] - paged["backward"] == 1_400_000 * (8 + 128) - 3 * 64 * 250_000
    pmc = bench.committed_pmc("C5", 64, 250_000)
    assert {"k_forward", "k_backward", "step"} <= set(pmc) and 0 < pmc["k_forward"]["l2_hit"] < 1
    assert bench.alg_bytes(32) == {"forward": 140, "backward": 132, "step": 272}
    # the roofline object: achieved = the counters' bytes per launch / the launch's duration, frac = that / 8 TB/s (<= 1 for
    # any real kernel); the algorithmic figure rides beside it, flagged, and may pass 1
    kern = {"backward": {"avg_ms": 0.160, "traffic_bytes": 1_020_000_000, "traffic_source": "x", "alg_GBps": 8200.0,
                         "requested_GBps": 6400.0, "frac_of_ceiling": 0.58, "ceiling": {"GBps": 11100.0}}}
    pd = {"backward": {"nnz": 10_000_000 * 12, "launches": 12}}
    r = bench.roofline_block(kern, "backward", bench.alg_bytes(32), pd, {"step": {"traffic_bytes": 1_500_000_000}}, 0.29, True)
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and r["traffic"] == 1_020_000_000
    assert r["achieved"] == pytest.approx(1.02e9 / 160e-6 / 1e9) and r["frac"] == pytest.approx(r["achieved"] / r["peak"]) and r["frac"] < 1
    assert r["algorithmic_frac"] == pytest.approx(8200.0 / 8000.0) and r["traffic_measured_in_this_run"] is True
    assert r["step"]["frac"] == pytest.approx(1.5e9 / 0.29e-3 / 8e12) and r["nnz_per_launch"] == 10_000_000
    r2 = bench.roofline_block({"backward": {"avg_ms": 0.2, "requested_bytes_per_launch": 8e8}}, "backward", bench.alg_bytes(32), pd, {}, 0.3, False)
    # no counter pass for a configuration: no HBM-side figure is claimed (the bytes the kernel ASKS for ride beside the empty roofline)
    assert r2["traffic"] is None and r2["frac"] is None and "requested" in r2["basis"]
    assert r2["requested_only"]["requested_bytes"] == 8e8 and r2["requested_only"]["requested_GBps"] == pytest.approx(8e8 / 0.2e-3 / 1e9)


# ---- the JVM side (jvm/HipSGD.scala + jvm/fmhip_jni.c): no JDK / scalac in this image, so the sources are checked
# ---- against each other and against the header instead of being compiled

_JNI_TYPES = {"Int": "jint", "Long": "jlong", "Double": "jdouble", "Array[Double]": "jdoubleArray", "Array[Long]": "jlongArray",
              "Array[Int]": "jintArray", "Array[Byte]": "jbyteArray", "Unit": "void"}


def _scala_natives(src):
    out = {}
    for m in re.finditer(r"@native\s+def\s+(\w+)\s*\(([^)]*)\)\s*:\s*([\w\[\]]+)", src):
        args = [a.split(":")[1].strip() for a in m.group(2).split(",") if a.strip()]
        out[m.group(1)] = (args, m.group(3))
    return out


def _jni_functions(src):
    out = {}
    for m in re.finditer(r"JNIEXPORT\s+(\w+)\s+JNI_FN\((\w+)\)\s*\(([^)]*)\)", src):
        args = [" ".join(a.split()[:-1]) for a in m.group(3).split(",")]      # "JNIEnv *env" -> "JNIEnv", "jint dev" -> "jint"
        assert args[:2] == ["JNIEnv", "jobject"], (m.group(2), args)
        out[m.group(2)] = (args[2:], m.group(1))
    return out


def test_jvm_natives_match_the_jni_shim_and_the_header():
    scala = open(os.path.join(ROOT, "jvm", "HipSGD.scala")).read()
    shim = open(os.path.join(ROOT, "jvm", "fmhip_jni.c")).read()
    hdr = open(os.path.join(ROOT, "include", "fmhip.h")).read()
    natives, jni = _scala_natives(scala), _jni_functions(shim)
    assert len(natives) >= 20
    assert set(natives) == set(jni), (set(natives) ^ set(jni))
    for name, (args, ret) in natives.items():
        assert [_JNI_TYPES[a] for a in args] == jni[name][0], name
        assert _JNI_TYPES[ret] == jni[name][1], name
    # every C-ABI symbol the shim calls is declared by the header
    declared = set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", hdr)) | set(re.findall(r"\b(fmhip_[a-z0-9_]+_t)\b", hdr))
    used = set(re.findall(r"\b(fmhip_[a-z0-9_]+)\b", re.sub(r"/\*.*?\*/", "", shim, flags=re.S))) - {"fmhip_jni"}
    assert used <= declared, used - declared
    # every HipSGD.<name>( call in the Scala source has a definition in the companion object, with that many arguments
    defs = {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
            for m in re.finditer(r"\bdef\s+(\w+)\s*\(([^)]*)\)", scala[scala.index("object HipSGD"):])}
    for m in re.finditer(r"HipSGD\.(\w+)\(", scala):
        assert m.group(1) in defs, m.group(1)
    for name, (args, _) in natives.items():
        for call in re.finditer(r"HipSGD\.%s\(([^()]*(?:\([^()]*\)[^()]*)*)\)" % name, scala):
            depth, n = 0, 1
            for ch in call.group(1):
                depth += ch in "([" 
                depth -= ch in ")]"
                n += ch == "," and depth == 0
            assert n == len(args) or (not call.group(1).strip() and not args), (name, call.group(0))
    # INTEGRATION.md states the count
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "%d natives" % len(natives) in integ


def test_jvm_class_has_no_duplicate_members():
    """The round-2 source declared `rank` twice (a constructor parameter and a var): scalac refuses that."""
    scala = open(os.path.join(ROOT, "jvm", "HipSGD.scala")).read()
    cls = scala[scala.index("class HipSGD"):scala.index("object HipSGD")]
    params = re.search(r"class HipSGD protected \(([^)]*)\)", cls, re.S).group(1)
    names = [p.split(":")[0].strip() for p in params.split(",")]
    body = cls[cls.index("extends FMLearn"):]
    depth, members = 0, []
    for line in body.splitlines():
        if depth == 1:
            m = re.match(r"\s*(?:@transient\s+)?(?:override\s+)?(?:private\s+|protected\s+)?(?:var|val|def)\s+(\w+)", line)
            if m:
                members.append(m.group(1))
        depth += line.count("{") - line.count("}")
    assert len(members) >= 8
    every = names + members
    assert len(every) == len(set(every)), sorted(n for n in every if every.count(n) > 1)
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", scala, flags=re.S))      # comments may hold "[lo, hi)"
    assert code.count("{") == code.count("}") and code.count("(") == code.count(")") and code.count("[") == code.count("]")


def test_bench_record_survives_a_kill_inside_an_optional_leg(tmp_path):
    """benchkit/emit.py: bench.py writes the WHOLE record as one JSON line as soon as the headline exists and re-writes it after
    every leg, each leg started only if the wall-clock budget covers its estimate.  Here a stand-in process (no GPU needed) emits
    a headline, one enriched line, then hangs in an "optional leg" with half a line on stdout; it is killed, and the last COMPLETE
    line still parses as a valid record — with the enrichment, without the leg that hung; a leg the budget cannot cover is
    recorded as skipped instead of started."""
    import json
    import signal
    import subprocess
    import time
    prog = tmp_path / "emit_then_hang.py"
    prog.write_text('''
import os, sys, time
sys.path.insert(0, %r)
from benchkit.emit import Budget, Emitter
b = Budget(30.0)
e = Emitter(1, b)
rec = {"metric": "nnz_per_sec_fm_sgd_training", "value": 1.0, "roofline": {"frac": 0.5}, "cpu_baseline": None}
e.emit(rec, "headline")
rec["cpu_baseline"] = b.run("cpu_baseline", 1.0, lambda: {"value": 2.0})
assert b.run("too_long", 1000.0, lambda: 1 / 0) is None          # never started: the estimate does not fit
e.emit(rec, "cpu_baseline")
os.write(1, b'{"metric": "half a li')                              # a leg that dies mid-write
time.sleep(600)
''' % ROOT)
    p = subprocess.Popen([sys.executable, str(prog)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    t0, data = time.time(), b""
    os.set_blocking(p.stdout.fileno(), False)
    while time.time() - t0 < 60 and b"half a li" not in data:
        chunk = p.stdout.read()
        data += chunk or b""
        time.sleep(0.05)
    p.send_signal(signal.SIGKILL)
    p.wait()
    assert b"half a li" in data, (data, p.stderr.read())
    from benchkit.emit import last_record
    rec = last_record(data.decode())
    assert rec["record"] == {"line": 2, "stage": "cpu_baseline", "final": False, "note": rec["record"]["note"]}
    assert rec["cpu_baseline"] == {"value": 2.0} and rec["roofline"]["frac"] == 0.5 and rec["value"] == 1.0
    assert "too_long" in rec["legs"]["skipped"] and "cpu_baseline" in rec["legs"]["seconds"] and rec["legs"]["time_budget_s"] == 30.0
    first = json.loads(data.decode().splitlines()[0])
    assert first["record"]["stage"] == "headline" and first["cpu_baseline"] is None and first["value"] == 1.0


def test_bench_roofline_says_what_bounds_the_step():
    """benchkit/roofline.py: the compulsory HBM bytes of a C3 step (every stream once, the hot pages once, one
    pass each over P, V and G) are ~0.25-0.3 GB = ~35 us at 8 TB/s — a fraction of the measured step — and an algorithmic
    fraction above 1 is labelled as a model that is not a bound."""
    import bench
    comp = bench.compulsory_hbm_bytes(32, 250_000, 8_000_000, 6_600_000, 90_000, 100_004, 4)
    assert comp["total"] == comp["streams"] + comp["xhot"] + comp["P_V_G_one_pass_each"] and 2.0e8 < comp["total"] < 3.5e8
    roof = {"algorithmic_frac": 1.31, "frac": 0.66}
    bench.annotate_roofline(roof, comp, 0.2415, 0.74)
    assert roof["compulsory_hbm_bytes_per_step"] == comp["total"] and 0.02 < roof["hbm_floor_ms"] < 0.05
    assert 0.1 < roof["hbm_floor_share_of_step"] < 0.2 and roof["step_ceiling_frac"] == 0.74
    assert roof["algorithmic_label"].startswith("model not a bound: tables cache-resident, hot block gathers nothing")
    roof2 = bench.annotate_roofline({"algorithmic_frac": 0.8}, comp, 0.3)
    assert "algorithmic_label" not in roof2 and "step_ceiling_frac" not in roof2


def test_host_arithmetic_under_the_sanitizers(tmp_path):
    """the library's pure host arithmetic — row shards, feature relabelling (one thread, private tables per
    thread, one table with atomic adds), a batch's range / fixup metadata incl. row-blocked pieces, the band-affine plan of the
    backward's ranges, the ALS level schedule, the data-parallel plan's cuts, interval edges, equal shares, update groups and compact intervals,
    and the host passes of the dataset build (validate_rows, choose_hot_block, split_hot_rows, forward_row_order, sort_rows_by_feature:
    float and double values, 1 and 4 threads with equal results; own_bitmaps)
    (sparkfm_amd/csrc/fmhip_host.cpp: the very translation unit libfmhip.so links) — compiled with g++ -fsanitize=address,undefined
    and driven over seeded random shapes by tests/host_arith_harness.cpp, which checks every function against the contract the
    device code relies on (each range in exactly one ascending run of the band plan, no two columns of an ALS level sharing a
    row, shares that tile their interval, a hot block without a feature stored twice in a row whose pages ascend, a split that
    loses no entry ...).  The GPU pool cannot run sanitizers; this index arithmetic needs no GPU."""
    import subprocess
    exe = str(tmp_path / "host_arith")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "host_arith_harness.cpp"), os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("no sanitizer runtime for g++ in this image")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    for seed in (20261005, 7, 99):
        r = subprocess.run([exe, str(seed), "25"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
        assert r.returncode == 0 and b"checks ok" in r.stdout, (seed, r.stderr.decode()[-3000:])
    # fmhip_step_backward's tiling rule (bw_window_step), exhaustively: n+1 in {1, 2, 7, 300}, every cut of [0, n+1) into 1 to 4
    # intervals, every order of them — descending accepted with kOwnLower, ascending with kOwnUpper, the window closed after the
    # last interval, any other order refused at its first wrong call with the window unchanged, finish above feature 0 refused,
    # a closed window refusing everything, hi = INT64_MAX taken as n+1; the refusals' texts byte for byte
    r = subprocess.run([exe, "window"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"), timeout=600)
    assert r.returncode == 0 and b"backward window" in r.stdout and b"checks ok" in r.stdout, r.stderr.decode()[-3000:]
    # the library itself links this translation unit (not a copy): the build lists it and the host entry points answer the same
    from sparkfm_amd import _build
    assert "fmhip_host.cpp" in _build.HIP_SOURCES


def test_cpp_mirror_of_the_reference_classes_compiles_and_reports_errors(tmp_path):
    """include/sparkfm.hpp: SparkFM's host classes (DataSet, FMModel, FMLearn, HipSGD / HipALS, FM + the fit loop) for a COMPILED
    host, header-only over the product C ABI (the reference is compiled JVM code; no JVM exists here).  CPU part: strict C++17,
    warnings as errors, only include/fmhip.h behind it; the model's shapes and defaults are the reference's
    (S/fm/FMModel.scala:17-22,29-31), and a library error arrives as sparkfm::Error carrying fmhip_last_error()."""
    import subprocess
    from helpers import build_cpp_mirror
    hpp = open(os.path.join(ROOT, "include", "sparkfm.hpp")).read()
    assert '#include "fmhip.h"' in hpp and "fmhip_experimental" not in hpp
    out = subprocess.check_output([build_cpp_mirror(tmp_path), "host"]).decode()
    assert "cpp_mirror host: checks ok" in out
