"""The backward's cost-ordered band plan (plan_bands, kWalkOrderColdFirst: the default) against the stream-order plan of
FMHIP_BWD_ORDER=0: scheduling only.  What a range computes and stores never depends on which wave walks it or when, and a launch
under the plan forms no wave sums, so EVERY BIT of the packed gradient and of the parameters after three steps must be equal,
and a second run must reproduce the first."""
import ctypes as C

import numpy as np
import pytest

from sparkfm_amd import _ffi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def problem(seed, rows, feats, k, nnz_lo, nnz_hi, permute_ids=False):
    from sparkfm_amd import synth
    d = synth.make_zipf(seed, rows, feats, nnz_lo, nnz_hi, zipf_s=1.05)
    col = d["col"]
    if permute_ids:           # ids NOT ranked by frequency: the expensive cold stretches lie anywhere in the stream
        col = np.random.default_rng(seed).permutation(feats).astype(col.dtype)[col]
    rng = np.random.default_rng(seed + 1)
    return dict(n1=feats, k=k, row_ptr=d["row_ptr"], col=col, val=d["val"].astype(np.float64), y=d["y"].astype(np.float64),
                w0=0.1, w=rng.normal(0, 0.05, feats), v=rng.normal(0, 0.05, (k, feats)))


def dataset(fmhip, a, batch_rows, order, monkeypatch):
    """the dataset with its band plan made under FMHIP_BWD_ORDER = order (None: the default); the plan is made when the
    dataset is built"""
    if order is None:
        monkeypatch.delenv("FMHIP_BWD_ORDER", raising=False)
    else:
        monkeypatch.setenv("FMHIP_BWD_ORDER", str(order))
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=batch_rows).cache()
    monkeypatch.delenv("FMHIP_BWD_ORDER", raising=False)
    return ds


def run(fmhip, ds, a, steps=3):
    """the packed gradient of every batch, then the parameters after `steps` SGD steps"""
    L = _ffi.load()
    fm = fmhip.FMModel(a["n1"] - 1, a["k"])
    fm.w0, fm.w, fm.v = a["w0"], a["w"], a["v"]
    out = []
    for b in range(ds.n_batches):
        gv, gw, g0, st = fm.batchGradient(ds, b)
        out += [np.asarray(gv).copy(), np.asarray(gw).copy(), np.float64(g0)]
    for j in range(steps):
        _ffi.check(L.fmhip_sgd_step(fm.handle, ds.handle, j % ds.n_batches, 0.02, 0.0, 1e-3, 1e-3, None))
    out += [np.float64(fm.w0), np.asarray(fm.w).copy(), np.asarray(fm.v).copy()]
    fm.close()
    return out


def same_bits(x, y, what):
    assert len(x) == len(y)
    for i, (p, q) in enumerate(zip(x, y)):
        p, q = np.ascontiguousarray(p), np.ascontiguousarray(q)
        assert p.shape == q.shape and p.dtype == q.dtype and p.tobytes() == q.tobytes(), (what, i)


# 20,000 x 2,000 Zipf in batches of 10,000 (some 3,000 ranges per batch: several rounds of workgroups per XCD list); the
# same in ONE batch (no dense hot block); ids not ranked by frequency; 2,000 x 300 in one batch: lists of a workgroup or
# two, and band runs — most columns are too short to be band-affine at 125 rows per band — that are empty
CASES = [
    ("zipf-k32", dict(seed=4700, rows=20_000, feats=2000, k=32, nnz_lo=10, nnz_hi=30), 10_000),
    ("zipf-k16-packed", dict(seed=4701, rows=20_000, feats=2000, k=16, nnz_lo=10, nnz_hi=30), 10_000),
    ("zipf-k64", dict(seed=4702, rows=20_000, feats=2000, k=64, nnz_lo=10, nnz_hi=30), 10_000),
    ("zipf-k32-one-batch-no-hot-block", dict(seed=4703, rows=20_000, feats=2000, k=32, nnz_lo=10, nnz_hi=30), 20_000),
    ("unranked-ids-k32", dict(seed=4704, rows=20_000, feats=2000, k=32, nnz_lo=10, nnz_hi=30, permute_ids=True), 10_000),
    ("small-k32", dict(seed=4705, rows=2000, feats=300, k=32, nnz_lo=40, nnz_hi=80), 2000),
    ("small-k16-packed", dict(seed=4706, rows=2000, feats=300, k=16, nnz_lo=40, nnz_hi=80), 2000),
]


@pytest.mark.parametrize("name,shape,batch_rows", CASES, ids=[c[0] for c in CASES])
def test_cost_ordered_lists_give_the_stream_order_s_bits(fmhip, monkeypatch, name, shape, batch_rows):
    a = problem(**shape)
    ds0 = dataset(fmhip, a, batch_rows, 0, monkeypatch)
    ds1 = dataset(fmhip, a, batch_rows, None, monkeypatch)
    for ds in (ds0, ds1):
        lay = ds.layout()
        assert lay["planned_ranges"] == lay["ranges"] >= 1024, lay       # every batch has a band plan
        assert (lay["hot_pages"] > 0) == (ds.n_batches > 1), lay         # the dense hot block is on exactly in the batched cases
    want = run(fmhip, ds0, a)
    got = run(fmhip, ds1, a)
    same_bits(got, want, name)
    same_bits(run(fmhip, ds1, a), got, (name, "second run"))
    ds0.unpersist()
    ds1.unpersist()


def test_feature_interval_launches_read_an_ascending_run(fmhip, monkeypatch):
    """Under the cost order a list's free part is dealt by cost; a feature-interval launch still reads the plan's INTERVAL form
    — every run ascending, clipped to the launch's window by binary search: forward + descending / ascending interval backwards
    must fill the packed gradient with the bits of the whole-batch backward (which walks the cost order) and of the stream-order
    plan's, over several cuts (inside hot columns, at column starts, around an empty interval)."""
    import torch
    from sparkfm_amd.distributed import HipEngine, torch_stream_handle
    L = _ffi.load()
    a = problem(seed=4710, rows=40_000, feats=3000, k=32, nnz_lo=10, nnz_hi=30)
    want = None
    for order in (0, None):
        ds = dataset(fmhip, a, 20_000, order, monkeypatch)
        fm = fmhip.FMModel(a["n1"] - 1, a["k"], stream=torch_stream_handle(0))
        fm.w0, fm.w, fm.v = a["w0"], a["w"], a["v"]
        lay = ds.layout()
        assert lay["planned_ranges"] == lay["ranges"] > 2048
        eng = HipEngine(fm, ds)

        def rebind():
            eng.grad.zero_()
            torch.cuda.synchronize()
            _ffi.check(L.fmhip_grad_bind(fm.handle, C.c_void_p(eng.grad.data_ptr())))

        eng.compute(1)
        torch.cuda.synchronize()
        if want is None:
            want = eng.grad.clone()
        assert torch.equal(eng.grad, want), order
        rebind()
        for cuts in ([0, 70, 3000], [0, 3, 64, 65, 700, 2999, 3000], [0, 1500, 1500, 3000], [0, 9, 400, 3000]):
            for ascending in (False, True):
                eng.forward(1)
                for i in (range(1, len(cuts)) if ascending else range(len(cuts) - 1, 0, -1)):
                    eng.backward(1, cuts[i - 1], cuts[i], finish=(i == 1))
                torch.cuda.synchronize()
                assert torch.equal(eng.grad, want), (order, cuts, ascending)
                rebind()
        eng.close()
        ds.unpersist()
        fm.close()
