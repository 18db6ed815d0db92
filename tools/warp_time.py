#!/usr/bin/env python3
"""WARP (include/fmhip_warp.h) against the best-of-C trainer (include/fmhip_bpr_adaptive.h) on the problem of tools/bpr_time.py and
tools/bpr_adaptive_time.py: a user block (an id feature and 9-29 history features per user), an item block (an id feature and 4-9
genre features), `interactions` observed (user, item) pairs with Zipf-popular items, n_neg = 1, k = 32.  For every batch size and
every C in {4, 16}: one handle and one model per sampler; each figure is a wall time to a device synchronise, the median of
`rounds` rounds after a warm-up of two epochs, the samplers taken turn by turn inside every round so that they see the same machine:

  resample    fmhip_bpr_resample_adaptive / fmhip_warp_resample (the two blocks' forwards, the sampler, the inverse map)
  epoch       HipBPR.learn (resample + every batch)

The WARP epoch does the best-of-C epoch's work plus one row gather per pair and one stream over the pairs' weights, minus the
candidates it does not look at after a chunk's first violator.  An earlier commit's best-of-C epoch on the same shapes is that
commit's tools/bpr_adaptive_time.py with the same arguments (the problem is generated from the same seed).

    python3 tools/warp_time.py [interactions] [users] [items] [batch_pairs,batch_pairs,...] [rounds] [samplers: auto,warp]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkfm_amd import DataSet, FMModel, HipBPR, _ffi  # noqa: E402

args = sys.argv[1:]
n_inter = int(args[0]) if len(args) > 0 else 1_000_000
n_users = int(args[1]) if len(args) > 1 else 20_000
n_items = int(args[2]) if len(args) > 2 else 5_000
batch_sizes = [int(x) for x in args[3].split(",")] if len(args) > 3 else [250_000, 32_768]
rounds = int(args[4]) if len(args) > 4 else 5
samplers = args[5].split(",") if len(args) > 5 else ["auto", "warp"]
COUNTS = (4, 16)
k, H, G = 32, 16384, 64
rng = np.random.default_rng(17)


def block(n, id0, lo, hi, f0, span):
    """n rows: the id feature id0 + j (value 1), then lo..hi distinct features of [f0, f0 + span) (span a power of two: an odd
    stride from a random start never repeats), value 1 / sqrt(their count)."""
    cnt = rng.integers(lo, hi + 1, n)
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(cnt + 1, out=ptr[1:])
    within = np.arange(ptr[-1], dtype=np.int64) - np.repeat(ptr[:-1], cnt + 1)
    start, stride = np.repeat(rng.integers(0, span, n), cnt + 1), np.repeat(rng.integers(0, span // 2, n) * 2 + 1, cnt + 1)
    col = np.where(within == 0, id0 + np.repeat(np.arange(n), cnt + 1), f0 + (start + (within - 1) * stride) % span).astype(np.int32)
    val = np.where(within == 0, 1.0, 1.0 / np.sqrt(np.repeat(cnt, cnt + 1))).astype(np.float32)
    return ptr, col, val


def zipf(n, size, s):
    p = 1.0 / np.arange(1, n + 1) ** s
    return rng.permutation(n)[rng.choice(n, size=size, p=p / p.sum())]


up, uc, uv = block(n_users, 0, 9, 29, n_users, H)
ip, ic, iv = block(n_items, n_users + H, 4, 9, n_users + H + n_items, G)
n1 = n_users + H + n_items + G
users = DataSet(up, uc, uv, np.zeros(n_users, np.float32), name="users", batch_rows=0).cache()
items = DataSet(ip, ic, iv, np.zeros(n_items, np.float32), name="items", batch_rows=0).cache()
key = np.unique(rng.integers(0, n_users, 2 * n_inter).astype(np.int64) * n_items + zipf(n_items, 2 * n_inter, 1.05))
key = np.sort(rng.choice(key, size=min(n_inter, len(key)), replace=False))
ctx_sorted, pos_sorted = (key // n_items).astype(np.int32), (key % n_items).astype(np.int32)
ptr = np.zeros(n_users + 1, np.int64)
np.cumsum(np.bincount(ctx_sorted, minlength=n_users), out=ptr[1:])
positives = [pos_sorted[ptr[u]:ptr[u + 1]] for u in range(n_users)]
eta, regw, regv = 0.02, 1e-4, 1e-4
L = _ffi.load()


def timed(fn, fm):
    _ffi.check(L.fmhip_synchronize(fm.handle))
    t = time.perf_counter()
    fn()
    _ffi.check(L.fmhip_synchronize(fm.handle))
    return time.perf_counter() - t


summary = lambda v: dict(median=float(np.median(v)) * 1e3, min=min(v) * 1e3, max=max(v) * 1e3)      # noqa: E731
out = dict(interactions=int(len(key)), users=n_users, items=n_items, k=k, features=n1, rounds=rounds, samplers=samplers, runs=[])
for batch_pairs in batch_sizes:
    names = [(s, c) for c in COUNTS for s in samplers]
    bprs, models = {}, {}
    for s, c in names:
        kw = dict(sampler="warp", margin=1.0) if s == "warp" else {}
        bprs[s, c] = HipBPR.run(users, items, positives, n_neg=1, batch_pairs=batch_pairs, seed=3, eta=eta, regw=regw, regv=regv, n_candidates=c, **kw)
        models[s, c] = FMModel(n1 - 1, k, seed=3, init_on_device=True)
    for n in names:      # warm-up: every kernel instance loaded, workspaces sized, the models away from their initial point
        for _ in range(2):
            bprs[n].learn(models[n])
    resample_s, epoch_s, stats = {n: [] for n in names}, {n: [] for n in names}, {}
    for r in range(rounds):
        t = 10 + r
        for n in names:
            resample_s[n].append(timed(lambda n=n: bprs[n].resample(t, models[n]), models[n]))
            stats[n] = bprs[n].sample_stats
        for n in names:
            epoch_s[n].append(timed(lambda n=n: bprs[n].learn(models[n]), models[n]))
    run = dict(batch_pairs=bprs[names[0]].batch_pairs, batches=bprs[names[0]].n_batches, pairs=bprs[names[0]].n_pairs,
               resample_ms={"%s_%d" % n: summary(v) for n, v in resample_s.items()},
               epoch_ms={"%s_%d" % n: summary(v) for n, v in epoch_s.items()},
               sample_stats={"%s_%d" % n: stats[n] for n in names})
    if "auto" in samplers and "warp" in samplers:
        run["warp_epoch_over_best_of_c_epoch"] = {"c_%d" % c: run["epoch_ms"]["warp_%d" % c]["median"] / run["epoch_ms"]["auto_%d" % c]["median"]
                                                  for c in COUNTS}
    out["runs"].append(run)
    for n in names:
        bprs[n].close()
        models[n].close()
print(json.dumps(out))
