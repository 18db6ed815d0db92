#!/usr/bin/env python3
"""Times fmhip_topk (FMModel.recommend): median of `--calls` calls after a warm-up, each a whole C-ABI call (the two forwards,
the candidates' table, the product with selection, the merge, the copy back).  Prints pairs/s, flop/s = 2 * Kp * B * M / t and
that as a fraction of the 157.3 TF f32-MFMA peak of an MI355X.

    python3 tools/topk_time.py --shape ml1m      6,040 x 3,706, 8 factors          (MovieLens-1M users x items)
    python3 tools/topk_time.py --shape square    100,000 x 100,000, 32 factors
    python3 tools/topk_time.py --shape latency   1 x 10,000,000, 32 factors        (bound by the candidates' table: GB/s beside it)
    python3 tools/topk_time.py --shape joined    4,096 x 16,384, 32 factors, AGAINST the route without this call: the 67 M
                                                 joined rows built on the host, uploaded (fmhip_rows_create_f32) and scored
                                                 (fmhip_predict) — the predict call alone and the whole route, as two numbers
    python3 tools/topk_time.py --shape BxMxk     anything else
Rows are synthetic: a context holds a user id and one side feature, a candidate an item id and one side feature (disjoint id
ranges), so a joined row is an ordinary row of four entries."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkfm_amd import DataSet, FMModel, _ffi  # noqa: E402

PEAK_F32_MFMA = 157.3e12
SHAPES = {"ml1m": (6040, 3706, 8), "square": (100_000, 100_000, 32), "latency": (1, 10_000_000, 32), "joined": (4096, 16384, 32)}


def side_rows(rng, n, id0, n_ids, feat0, n_feat):
    col = np.empty((n, 2), np.int32)
    col[:, 0] = id0 + np.arange(n) % n_ids
    col[:, 1] = feat0 + rng.integers(0, n_feat, n)
    val = np.ones((n, 2), np.float32)
    val[:, 1] = rng.uniform(0.5, 1.0, n).astype(np.float32)
    return np.arange(0, 2 * n + 1, 2, dtype=np.int64), col.reshape(-1), val.reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="ml1m")
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    B, M, k = SHAPES[a.shape] if a.shape in SHAPES else (int(x) for x in a.shape.split("x"))
    rng = np.random.default_rng(1)
    nu, ni, nf = min(B, 1 << 20), min(M, 1 << 20), 64
    n1 = nu + nf + ni + nf
    ctx = side_rows(rng, B, 0, nu, nu, nf)
    cand = side_rows(rng, M, nu + nf, ni, nu + nf + ni, nf)
    fm = FMModel(n1 - 1, k, init_stdev=0.1, seed=5, init_on_device=True)
    dc = DataSet(*ctx, np.zeros(B, np.float32), scoring=True).cache()
    dd = DataSet(*cand, np.zeros(M, np.float32), scoring=True).cache()
    L = _ffi.load()
    na, nk, kp = _ffi.C.c_int64(), _ffi.C.c_int32(), _ffi.C.c_int32()
    _ffi.check(L.fmhip_model_info(fm.handle, _ffi.C.byref(na), _ffi.C.byref(nk), _ffi.C.byref(kp)))
    Kp = kp.value
    fm.recommend(dc, dd, a.topk)                                     # warm-up: kernels loaded, pools filled
    t = []
    for _ in range(max(a.calls, 5)):
        t0 = time.perf_counter()
        idx, sc = fm.recommend(dc, dd, a.topk)
        t.append(time.perf_counter() - t0)
    med = float(np.median(t))
    flops = 2.0 * Kp * B * M / med
    line = ("%s: %d x %d, %d factors (Kp = %d), K = %d: fmhip_topk median of %d calls %.3f ms (min %.3f), %.3g pairs/s, %.2f Tflop/s = %.1f %% of "
            "the f32-MFMA peak" % (a.shape, B, M, k, Kp, a.topk, len(t), med * 1e3, min(t) * 1e3, B * M / med, flops / 1e12, 100 * flops / PEAK_F32_MFMA))
    if B <= 64:
        line += "; candidates' table %.2f GB: %.1f GB/s" % (M * Kp * 4 / 1e9, M * Kp * 4 / 1e9 / med)
    print(line, flush=True)
    if a.shape != "joined":
        return
    # the route without fmhip_topk: every (context, candidate) pair as one joined row of four entries
    t0 = time.perf_counter()
    cc, cv = ctx[1].reshape(B, 2), ctx[2].reshape(B, 2)
    dcol, dval = cand[1].reshape(M, 2), cand[2].reshape(M, 2)
    col = np.empty((B, M, 4), np.int32)
    val = np.empty((B, M, 4), np.float32)
    col[:, :, :2], col[:, :, 2:] = cc[:, None, :], dcol[None, :, :]
    val[:, :, :2], val[:, :, 2:] = cv[:, None, :], dval[None, :, :]
    ptr = np.arange(0, 4 * B * M + 1, 4, dtype=np.int64)
    t_build = time.perf_counter() - t0
    t0 = time.perf_counter()
    dj = DataSet(ptr, col.reshape(-1), val.reshape(-1), np.zeros(B * M, np.float32), scoring=True).cache()
    t_upload = time.perf_counter() - t0
    out = np.empty(B * M)
    _ffi.check(L.fmhip_predict(fm.handle, dj.handle, _ffi.ptr(out)))   # warm-up
    tp = []
    for _ in range(3):
        t0 = time.perf_counter()
        _ffi.check(L.fmhip_predict(fm.handle, dj.handle, _ffi.ptr(out)))
        tp.append(time.perf_counter() - t0)
    t_pred = float(np.median(tp))
    # the two routes rank alike (same scores up to fp32 rounding): the top candidate's joined-row prediction is the row's maximum
    full = out.reshape(B, M)
    worst = float(np.max(full.max(axis=1) - full[np.arange(B), idx[:, 0]]))
    print("joined-row route: build %.2f s + upload %.2f s + fmhip_predict %.3f s = %.2f s end to end; fmhip_topk %.4f s: %.0f x faster than the "
          "fmhip_predict call alone, %.0f x end to end (largest gap between a row's best joined-row prediction and its top-1's: %.2e)"
          % (t_build, t_upload, t_pred, t_build + t_upload + t_pred, med, t_pred / med, (t_build + t_upload + t_pred) / med, worst), flush=True)


if __name__ == "__main__":
    main()
