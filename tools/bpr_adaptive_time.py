#!/usr/bin/env python3
"""Adaptive negatives of the BPR trainer (include/fmhip_bpr_adaptive.h) against the uniform trainer, on the problem of
tools/bpr_time.py: a user block (an id feature and 9-29 history features per user), an item block (an id feature and 4-9 genre
features), `interactions` observed (user, item) pairs with Zipf-popular items, n_neg = 1, k = 32.  One handle and one model per
n_candidates in {1, 4, 16}; each figure is a wall time to a device synchronise, the median of `rounds` rounds after a warm-up, the
three counts taken turn by turn inside every round so that they see the same machine:

  resample    n_candidates = 1: fmhip_bpr_resample (uniform), and fmhip_bpr_resample_adaptive beside it (the two blocks' forwards +
              the adaptive sampler at one candidate); n_candidates > 1: fmhip_bpr_resample_adaptive
  epoch       HipBPR.learn (resample + every batch).  n_candidates = 1 takes the uniform trainer's code path unchanged: it is the
              uniform epoch every other column stands beside.

    python3 tools/bpr_adaptive_time.py [interactions] [users] [items] [batch_pairs] [rounds]"""
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
batch_pairs = int(args[3]) if len(args) > 3 else 250_000
rounds = int(args[4]) if len(args) > 4 else 5
COUNTS = (1, 4, 16)
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
bprs = {c: HipBPR.run(users, items, positives, n_neg=1, batch_pairs=batch_pairs, seed=3, eta=eta, regw=regw, regv=regv, n_candidates=c)
        for c in COUNTS}
models = {c: FMModel(n1 - 1, k, seed=3, init_on_device=True) for c in COUNTS}


def timed(fn, fm):
    _ffi.check(L.fmhip_synchronize(fm.handle))
    t = time.perf_counter()
    fn()
    _ffi.check(L.fmhip_synchronize(fm.handle))
    return time.perf_counter() - t


# warm-up: two epochs each (every kernel instance loaded, workspaces sized, the models away from their initial point)
for c in COUNTS:
    for _ in range(2):
        bprs[c].learn(models[c])
    bprs[c].resample(7, models[c])
bprs[1].resample(7)

resample_s = {("uniform" if c == 0 else "adaptive_%d" % c): [] for c in (0,) + COUNTS}
epoch_s = {c: [] for c in COUNTS}
stats = {}
for r in range(rounds):
    t = 10 + r
    resample_s["uniform"].append(timed(lambda: bprs[1].resample(t), models[1]))
    for c in COUNTS:
        resample_s["adaptive_%d" % c].append(timed(lambda c=c: bprs[c].resample(t, models[c]), models[c]))
        stats[c] = bprs[c].sample_stats
    for c in COUNTS:
        epoch_s[c].append(timed(lambda c=c: bprs[c].learn(models[c]), models[c]))

summary = lambda v, scale: dict(median=float(np.median(v)) * scale, min=min(v) * scale, max=max(v) * scale)      # noqa: E731
out = dict(interactions=int(len(key)), pairs=bprs[1].n_pairs, users=n_users, items=n_items, k=k, features=n1, batch_pairs=bprs[1].batch_pairs,
           batches=bprs[1].n_batches, rounds=rounds, nnz_blocks=int(users.nnz + items.nnz),
           resample_ms={n: summary(v, 1e3) for n, v in resample_s.items()},
           epoch_ms={"n_candidates_%d" % c: summary(v, 1e3) for c, v in epoch_s.items()},
           sample_stats={"n_candidates_%d" % c: stats[c] for c in COUNTS},
           pair_logloss={"n_candidates_%d" % c: bprs[c].computePairLogLoss(models[c]) for c in COUNTS})
uni = out["epoch_ms"]["n_candidates_1"]["median"]
out["epoch_over_uniform_epoch"] = {"n_candidates_%d" % c: out["epoch_ms"]["n_candidates_%d" % c]["median"] / uni for c in COUNTS}
out["candidate_row_bytes"] = {"n_candidates_%d" % c: bprs[c].n_pairs * c * 32 * 4 for c in COUNTS}
print(json.dumps(out))
