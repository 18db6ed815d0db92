#!/usr/bin/env python3
"""Times fmhip_rank (FMModel.rankOf) against the route without it: fmhip_pair_scores in chunks of contexts (the B x M scores
travel to the host as doubles) plus numpy's rank of every relevant row on the host.  Both routes are whole calls, timed with a
host clock (each ends in a device synchronise); median of `--calls` after a warm-up.  The two routes' ranks are compared.

    python3 tools/rank_time.py --shape loo     6,040 x 3,706, 32 factors: leave-one-out, one held-out item per user, the user's
                                               other ratings (165 each, MovieLens-1M's mean) excluded from the ranking
    python3 tools/rank_time.py --shape big     4,096 x 1,000,000, 32 factors, one relevant row per context, no exclusions; the
                                               baseline moves 33 GB: it is timed on --baseline-contexts contexts (default 256) and
                                               scaled by B / that — its cost is per context, chunk by chunk
    python3 tools/rank_time.py --shape BxMxk   anything else (one relevant row per context, no exclusions)
Beside the times: the call's pairs/s, flop/s = 2 * Kp * nq * M / t and that as a share of the 157.3 TF f32-MFMA peak of an MI355X
— a WHOLE-CALL rate (two forwards, the candidates' table, three kernels, the copies), not the sweep kernel's own; for that run
    rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/rank_time.py --shape big --no-baseline
and divide 2 * Kp * nq * M by k_pair_rank's time.
Rows are synthetic, as tools/topk_time.py's."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkfm_amd import DataSet, FMModel, _ffi  # noqa: E402

PEAK_F32_MFMA = 157.3e12
SHAPES = {"loo": (6040, 3706, 32), "big": (4096, 1_000_000, 32)}


def side_rows(rng, n, id0, n_ids, feat0, n_feat):
    col = np.empty((n, 2), np.int32)
    col[:, 0] = id0 + np.arange(n) % n_ids
    col[:, 1] = feat0 + rng.integers(0, n_feat, n)
    val = np.ones((n, 2), np.float32)
    val[:, 1] = rng.uniform(0.5, 1.0, n).astype(np.float32)
    return np.arange(0, 2 * n + 1, 2, dtype=np.int64), col.reshape(-1), val.reshape(-1)


def host_ranks(fm, dc, dd, rel, ex, c0, c1, chunk):
    """the parent's route for the contexts [c0, c1): pairScores chunk by chunk, numpy's rank of every relevant row"""
    out = []
    for lo in range(c0, c1, chunk):
        hi = min(lo + chunk, c1)
        S = fm.pairScores(dc, dd, lo, hi)
        for c in range(lo, hi):
            s = S[c - lo]
            if ex is not None:
                s = s.copy()
                s[ex[c]] = -np.inf                     # (scores are finite here; the held-out row is never excluded)
            r = []
            for t in rel[c]:
                st = s[t]
                r.append(int((s > st).sum() + (s[:t] == st).sum()))
            out.append(np.array(r, np.int32))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="loo")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--baseline-contexts", type=int, default=0, help="time the baseline on this many contexts and scale (0: all; big: 256)")
    ap.add_argument("--chunk-floats", type=int, default=1 << 25, help="scores per pairScores call of the baseline")
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
    rel = [np.array([t]) for t in rng.integers(0, M, B)]
    ex = None
    if a.shape == "loo":
        ex = []
        for c in range(B):
            e = np.unique(rng.integers(0, M, 170))
            ex.append(e[e != rel[c][0]][:165])
    L = _ffi.load()
    na, nk, kp = _ffi.C.c_int64(), _ffi.C.c_int32(), _ffi.C.c_int32()
    _ffi.check(L.fmhip_model_info(fm.handle, _ffi.C.byref(na), _ffi.C.byref(nk), _ffi.C.byref(kp)))
    Kp, nq = kp.value, sum(len(r) for r in rel)
    fm.rankOf(dc, dd, rel, exclude=ex)                               # warm-up: kernels loaded, pools filled
    t = []
    for _ in range(max(a.calls, 5)):
        t0 = time.perf_counter()
        ranks = fm.rankOf(dc, dd, rel, exclude=ex)
        t.append(time.perf_counter() - t0)
    med = float(np.median(t))
    # the C-ABI call alone, on arrays prepared once (rankOf also sorts and flattens the per-context lists, in numpy)
    rptr, ridx = _ffi.row_lists(rel, B, M, "relevant")
    eptr, eidx = _ffi.row_lists(ex, B, M, "exclude") if ex is not None else (None, None)
    out = np.empty(nq, np.int32)
    tc = []
    for _ in range(max(a.calls, 5)):
        t0 = time.perf_counter()
        _ffi.check(L.fmhip_rank(fm.handle, dc.handle, dd.handle, _ffi.ptr(rptr), _ffi.ptr(ridx), _ffi.ptr(eptr), _ffi.ptr(eidx), _ffi.ptr(out), None))
        tc.append(time.perf_counter() - t0)
    assert np.array_equal(out, np.concatenate(ranks))
    flops = 2.0 * Kp * nq * M / med
    n_ex = 0 if ex is None else sum(len(e) for e in ex)
    print("%s: %d contexts x %d candidates, %d factors (Kp = %d), %d queries, %d exclusions: rankOf median of %d calls %.3f ms (min %.3f), "
          "of which fmhip_rank itself %.3f ms; %.3g pairs/s, whole-call %.2f Tflop/s = %.1f %% of the f32-MFMA peak"
          % (a.shape, B, M, k, Kp, nq, n_ex, len(t), med * 1e3, min(t) * 1e3, float(np.median(tc)) * 1e3, nq * M / med, flops / 1e12,
             100 * flops / PEAK_F32_MFMA), flush=True)
    if a.no_baseline:
        return
    nb = a.baseline_contexts or (256 if a.shape == "big" else B)
    nb = min(nb, B)
    chunk = max(1, a.chunk_floats // M)
    host_ranks(fm, dc, dd, rel, ex, 0, min(chunk, nb), chunk)        # warm-up
    tb = []
    for _ in range(3 if nb * M <= 1 << 28 else 1):
        t0 = time.perf_counter()
        ref = host_ranks(fm, dc, dd, rel, ex, 0, nb, chunk)
        tb.append(time.perf_counter() - t0)
    base = float(np.median(tb)) * B / nb
    same = all(np.array_equal(ranks[c], ref[c]) for c in range(nb))
    print("pairScores + numpy route: %.3f s for %d contexts in chunks of %d (%.2f GB of doubles)%s = %.3f s for all %d; rankOf %.4f s: %.1f x; "
          "ranks of the two routes %s"
          % (float(np.median(tb)), nb, chunk, nb * M * 8 / 1e9, "" if nb == B else ", scaled by %d / %d" % (B, nb), base, B, med, base / med,
             "agree" if same else "DIFFER"), flush=True)
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
