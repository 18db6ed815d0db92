#!/usr/bin/env python3
"""What the sampled softmax (include/fmhip_softmax.h) costs an epoch of the BPR trainer, on the recommender-shaped problem of
tools/bpr_time.py (the same generator and seed: a user block, an item block, distinct (user, item) interactions with Zipf-popular
items, k = 32).  For every (n_neg, batch_pairs, loss) of {4, 16} x {large, small} x {"logistic", "softmax"}, pairs = n_neg *
interactions held at `pairs`: the wall time of HipBPR.learn — the draw of every pair, the inverse map of every batch, every batch's
step — to a device synchronise, the median (min - max) of `rounds` epochs after two warm-up epochs, each configuration on a fresh
handle and model.  The softmax adds one pre-pass launch per batch and swaps the pairs' finish for its given-residual instance.
One JSON line.

    python3 tools/bpr_softmax_time.py [pairs] [users] [items] [rounds] [large_batch_pairs] [small_batch_pairs]
Run from a checkout whose HipBPR has no softmax it measures the logistic configurations alone: the parent's figures, for the same
session."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkfm_amd import DataSet, FMModel, HipBPR, _ffi  # noqa: E402

args = sys.argv[1:]
n_pairs = int(args[0]) if len(args) > 0 else 1_000_000
n_users = int(args[1]) if len(args) > 1 else 20_000
n_items = int(args[2]) if len(args) > 2 else 5_000
rounds = int(args[3]) if len(args) > 3 else 27
large = int(args[4]) if len(args) > 4 else 250_000       # 4 batches of 1 M pairs; a multiple of 16
small = int(args[5]) if len(args) > 5 else 32_768        # 31 batches
k, H, G = 32, 16384, 64
rng = np.random.default_rng(17)


def block(n, id0, lo, hi, f0, span):
    """bpr_time.py's: n rows, the id feature id0 + j (value 1), then lo..hi distinct features of [f0, f0 + span)."""
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
most = n_pairs // 4
key_all = np.unique(rng.integers(0, n_users, 2 * most).astype(np.int64) * n_items + zipf(n_items, 2 * most, 1.05))
L = _ffi.load()
losses = ("logistic", "softmax") if hasattr(HipBPR, "computeSoftmaxLoss") else ("logistic",)
out = dict(pairs=n_pairs, users=n_users, items=n_items, k=k, rounds=rounds, losses=list(losses), epoch_ms={}, batches={})
for n_neg in (4, 16):
    n_inter = n_pairs // n_neg
    key = np.sort(np.random.default_rng(18).choice(key_all, size=min(n_inter, len(key_all)), replace=False))
    ctx_sorted, pos_sorted = (key // n_items).astype(np.int32), (key % n_items).astype(np.int32)
    ptr = np.zeros(n_users + 1, np.int64)
    np.cumsum(np.bincount(ctx_sorted, minlength=n_users), out=ptr[1:])
    positives = [pos_sorted[ptr[u]:ptr[u + 1]] for u in range(n_users)]
    for bp in (large, small):
        for loss in losses:
            bpr = HipBPR.run(users, items, positives, n_neg=n_neg, batch_pairs=bp, seed=3, eta=0.02, regw=1e-4, regv=1e-4, loss=loss)
            fm = FMModel(n1 - 1, k, seed=3, init_on_device=True)
            times = []
            for r in range(2 + rounds):
                _ffi.check(L.fmhip_synchronize(fm.handle))
                t = time.perf_counter()
                bpr.learn(fm)
                _ffi.check(L.fmhip_synchronize(fm.handle))
                times.append((time.perf_counter() - t) * 1e3)
            name = "%s_n%d_b%d" % (loss, n_neg, bpr.n_batches)
            out["epoch_ms"][name] = dict(median=float(np.median(times[2:])), min=min(times[2:]), max=max(times[2:]))
            out["batches"][name] = dict(pairs=bpr.n_pairs, batches=bpr.n_batches)
            bpr.close()
            fm.close()
print(json.dumps(out))
