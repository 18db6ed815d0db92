#!/usr/bin/env python3
"""The BPR trainer (include/fmhip_bpr.h) against the routes it replaces, on one recommender-shaped problem: a user block (an id
feature and 9-29 history features per user), an item block (an id feature and 4-9 genre features), `interactions` observed (user,
item) pairs with Zipf-popular items, n_neg = 1, k = 32.  Three measurements, each to a device synchronise, medians after a warm-up:

  resample    fmhip_bpr_resample: the device sampler + the inverse map of every batch + the counts' read-back, per epoch
  step        one fmhip_bpr_step against one flat pair step (fmhip_sgd_step, pairing on) on expand() of the SAME pairs
  epoch       HipBPR.learn (resample + every batch) against the only route without it: negatives drawn on the host in numpy, the
              joined rows of both sides of every pair built, a new DataSet made and cached (CSR, transposes, upload), one
              HipSGD(pairs=True) epoch, the dataset freed — all of it inside the timed region, as it recurs every epoch

    python3 tools/bpr_time.py [interactions] [users] [items] [batch_pairs] [rounds]
The relational step walks both whole blocks every batch, so it pays off when a batch's rows (2 * batch_pairs) outnumber the blocks'
rows (users + items): run it once on each side of that."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkfm_amd import DataSet, FMModel, HipBPR, HipSGD, _ffi  # noqa: E402

args = sys.argv[1:]
n_inter = int(args[0]) if len(args) > 0 else 1_000_000
n_users = int(args[1]) if len(args) > 1 else 20_000
n_items = int(args[2]) if len(args) > 2 else 5_000
batch_pairs = int(args[3]) if len(args) > 3 else 250_000
rounds = int(args[4]) if len(args) > 4 else 3
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
# distinct (user, item) interactions: uniform users, Zipf items
key = np.unique(rng.integers(0, n_users, 2 * n_inter).astype(np.int64) * n_items + zipf(n_items, 2 * n_inter, 1.05))
key = np.sort(rng.choice(key, size=min(n_inter, len(key)), replace=False))
ctx_sorted, pos_sorted = (key // n_items).astype(np.int32), (key % n_items).astype(np.int32)
ptr = np.zeros(n_users + 1, np.int64)
np.cumsum(np.bincount(ctx_sorted, minlength=n_users), out=ptr[1:])
positives = [pos_sorted[ptr[u]:ptr[u + 1]] for u in range(n_users)]
eta, regw, regv = 0.02, 1e-4, 1e-4
bpr = HipBPR.run(users, items, positives, n_neg=1, batch_pairs=batch_pairs, seed=3, eta=eta, regw=regw, regv=regv)
L = _ffi.load()
n_pairs, steps = bpr.n_pairs, bpr.n_batches
models = {name: FMModel(n1 - 1, k, seed=3, init_on_device=True) for name in ("bpr", "flat", "host_route")}


def sync(fm):
    _ffi.check(L.fmhip_synchronize(fm.handle))


def timed(fn, fm):
    sync(fm)
    t = time.perf_counter()
    fn()
    sync(fm)
    return time.perf_counter() - t


def join(ctx, pos, neg, batch_rows):
    """The flat DataSet of the pairs: row 2p = user ++ positive (label 1), row 2p + 1 = user ++ negative (label 0)."""
    n = 2 * len(ctx)
    u = np.repeat(ctx.astype(np.int64), 2)
    i = np.empty(n, np.int64)
    i[0::2], i[1::2] = pos, neg
    lens = [up[u + 1] - up[u], ip[i + 1] - ip[i]]
    row_ptr = np.zeros(n + 1, np.int64)
    np.cumsum(lens[0] + lens[1], out=row_ptr[1:])
    col, val = np.empty(row_ptr[-1], np.int32), np.empty(row_ptr[-1], np.float32)
    at = row_ptr[:-1].copy()
    for (p_, c_, v_, mp), ln in zip(((up, uc, uv, u), (ip, ic, iv, i)), lens):
        within = np.arange(ln.sum(), dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln)
        src, dst = np.repeat(p_[mp], ln) + within, np.repeat(at, ln) + within
        col[dst], val[dst] = c_[src], v_[src]
        at += ln
    y = np.zeros(n, np.float32)
    y[0::2] = 1.0
    return DataSet(row_ptr, col, val, y, name="pairs", batch_rows=batch_rows)


def host_negatives(gen, ctx, pos_key):
    """A row outside the user's positives per pair, by rejection in numpy (a binary search over the sorted (user, item) keys)."""
    neg = gen.integers(0, n_items, len(ctx))
    while True:
        k_ = ctx.astype(np.int64) * n_items + neg
        at = np.minimum(np.searchsorted(pos_key, k_), len(pos_key) - 1)
        bad = np.flatnonzero(pos_key[at] == k_)
        if not len(bad):
            return neg
        neg[bad] = gen.integers(0, n_items, len(bad))


def host_route_epoch(t, parts):
    fm = models["host_route"]
    t0 = time.perf_counter()
    neg = host_negatives(np.random.default_rng([3, t]), bpr.inter_ctx, key)
    t1 = time.perf_counter()
    ds = join(bpr.inter_ctx, bpr.inter_cand, neg, 2 * bpr.batch_pairs)
    t2 = time.perf_counter()
    ds.cache()
    t3 = time.perf_counter()
    HipSGD(eta=eta, regw=regw, regv=regv, loss="logistic", pairs=True).learn(fm, ds)
    sync(fm)
    t4 = time.perf_counter()
    ds.unpersist()
    parts.append(dict(sample_s=t1 - t0, join_s=t2 - t1, dataset_s=t3 - t2, train_s=t4 - t3))


# ---- resample ------------------------------------------------------------------------------------------------------------------
bpr.resample(0)
resample_s = [timed(lambda t=t: bpr.resample(t), models["bpr"]) for t in range(1, 1 + max(rounds, 3))]
stats = bpr.sample_stats

# ---- step: the same pairs through both steps ---------------------------------------------------------------------------------------
flat = bpr.expand().cache()
sgd = HipSGD(eta=eta, regw=regw, regv=regv, loss="logistic", pairs=True)


def bpr_steps():
    for b in range(steps):
        bpr.step(models["bpr"], b, want_stats=False)


def flat_steps():
    for b in range(steps):
        sgd.step(models["flat"], flat, b, want_stats=False)


for fn, name in ((bpr_steps, "bpr"), (flat_steps, "flat")):      # warm-up: every kernel instance loaded, tables touched
    timed(fn, models[name])
    timed(fn, models[name])
step_s = dict(bpr=[], flat=[])
for _ in range(max(rounds, 3)):
    step_s["bpr"].append(timed(bpr_steps, models["bpr"]) / steps)
    step_s["flat"].append(timed(flat_steps, models["flat"]) / steps)
nnz_flat_per_batch = flat.nnz / steps
flat.unpersist()

# ---- epoch: HipBPR.learn against the host route -------------------------------------------------------------------------------------
epoch_s, parts = dict(bpr=[], host_route=[]), []
host_route_epoch(0, [])                                                  # warm-up
for r in range(rounds):
    epoch_s["bpr"].append(timed(lambda: bpr.learn(models["bpr"]), models["bpr"]))
    epoch_s["host_route"].append(timed(lambda r=r: host_route_epoch(1 + r, parts), models["host_route"]))

med = lambda x: float(np.median(x))      # noqa: E731
out = dict(interactions=int(len(key)), pairs=n_pairs, users=n_users, items=n_items, k=k, features=n1, batch_pairs=bpr.batch_pairs, batches=steps,
           batch_rows=2 * bpr.batch_pairs, block_rows=n_users + n_items, rounds=rounds, nnz_blocks=int(users.nnz + items.nnz),
           nnz_flat_per_batch=nnz_flat_per_batch, sample_attempts=stats["attempts"], sample_forced=stats["forced"],
           resample_ms=dict(median=med(resample_s) * 1e3, min=min(resample_s) * 1e3, max=max(resample_s) * 1e3),
           step_ms={n: dict(median=med(v) * 1e3, min=min(v) * 1e3, max=max(v) * 1e3) for n, v in step_s.items()},
           epoch_s={n: dict(median=med(v), min=min(v), max=max(v)) for n, v in epoch_s.items()},
           host_route_parts_s={n: med([p[n] for p in parts]) for n in parts[0]})
out["flat_step_over_bpr_step"] = out["step_ms"]["flat"]["median"] / out["step_ms"]["bpr"]["median"]
out["host_route_epoch_over_bpr_epoch"] = out["epoch_s"]["host_route"]["median"] / out["epoch_s"]["bpr"]["median"]
print(json.dumps(out))
