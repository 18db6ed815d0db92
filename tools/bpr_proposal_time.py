#!/usr/bin/env python3
"""What the weighted proposal (include/fmhip_proposal.h) costs an epoch of the BPR trainer, on the recommender-shaped problem of
tools/bpr_time.py (the same generator and seed: a user block, an item block, distinct (user, item) interactions with Zipf-popular
items, n_neg = 1, k = 32).  For every (proposal, n_candidates) of {"uniform", "popularity"} x {1, 16}: the wall time of
HipBPR.learn — the draw of every pair, the inverse map of every batch, every batch's step — to a device synchronise, the median
(min - max) of `rounds` epochs after two warm-up epochs, each configuration on a fresh handle and model.  One JSON line.

    python3 tools/bpr_proposal_time.py [interactions] [users] [items] [batch_pairs] [rounds]
Run from a checkout whose HipBPR has no `negatives` keyword it measures the uniform configurations alone: the parent's figures,
for the same session."""
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
rounds = int(args[4]) if len(args) > 4 else 7
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
key = np.unique(rng.integers(0, n_users, 2 * n_inter).astype(np.int64) * n_items + zipf(n_items, 2 * n_inter, 1.05))
key = np.sort(rng.choice(key, size=min(n_inter, len(key)), replace=False))
ctx_sorted, pos_sorted = (key // n_items).astype(np.int32), (key % n_items).astype(np.int32)
ptr = np.zeros(n_users + 1, np.int64)
np.cumsum(np.bincount(ctx_sorted, minlength=n_users), out=ptr[1:])
positives = [pos_sorted[ptr[u]:ptr[u + 1]] for u in range(n_users)]
L = _ffi.load()
proposals = ("uniform", "popularity") if hasattr(HipBPR, "NEGATIVES") else ("uniform",)
out = dict(interactions=int(len(key)), users=n_users, items=n_items, k=k, batch_pairs=batch_pairs, rounds=rounds, proposals=list(proposals),
           epoch_ms={}, sample={})
for n_cand in (1, 16):
    for proposal in proposals:
        kw = dict(negatives=proposal) if len(proposals) > 1 else {}
        bpr = HipBPR.run(users, items, positives, n_neg=1, batch_pairs=batch_pairs, seed=3, eta=0.02, regw=1e-4, regv=1e-4, n_candidates=n_cand, **kw)
        fm = FMModel(n1 - 1, k, seed=3, init_on_device=True)
        times = []
        for r in range(2 + rounds):
            _ffi.check(L.fmhip_synchronize(fm.handle))
            t = time.perf_counter()
            bpr.learn(fm)
            _ffi.check(L.fmhip_synchronize(fm.handle))
            times.append((time.perf_counter() - t) * 1e3)
        name = "%s_C%d" % (proposal, n_cand)
        out["epoch_ms"][name] = dict(median=float(np.median(times[2:])), min=min(times[2:]), max=max(times[2:]))
        out["sample"][name] = bpr.resample(99, fm if n_cand > 1 else None)
        out["batches"] = bpr.n_batches
        bpr.close()
        fm.close()
print(json.dumps(out))
