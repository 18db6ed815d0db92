#!/usr/bin/env python3
"""A relational step (include/fmhip_relational.h) against the flat step on expand() of the same data: fmhip_relational_sgd_epoch
and fmhip_sgd_epoch on the same model shape, alternated in one process after a warm-up, each epoch timed to a device synchronise.
The data is a recommender's: a user block (an id feature and 19-59 history features per user: 20-60 nonzeros), an item block (an
id feature and 4-9 genre features: 5-10 nonzeros), Zipf mappings (popular users and items), no plain part; k = 32, 250 k rows per
batch.  Beside the times it prints the byte model of both steps (a walk moves 4 Kp + 12 B per stored nonzero; forward
and backward each walk their stream once) and the flat step's kernel breakdown (HIP events, fmhip_profile_*).
    python3 tools/relational_time.py [rows] [users] [items] [rounds] [--flat-only]
--flat-only touches nothing of the relational interface but expand(): the flat step alone.
The relational kernels' own times come from a kernel trace of this script in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/relational_time.py 500000 100000 20000 2"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkfm_amd import FMModel, Relation, RelationalData, _ffi  # noqa: E402

args = [x for x in sys.argv[1:] if not x.startswith("--")]
flat_only = "--flat-only" in sys.argv
rows = int(args[0]) if len(args) > 0 else 1_000_000
n_users = int(args[1]) if len(args) > 1 else 100_000
n_items = int(args[2]) if len(args) > 2 else 20_000
rounds = int(args[3]) if len(args) > 3 else 5
k, batch_rows, H, G = 32, 250_000, 16384, 64
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
    return rng.permutation(n)[rng.choice(n, size=size, p=p / p.sum())].astype(np.int32)


users = Relation(block(n_users, 0, 19, 59, n_users, H), zipf(n_users, rows, 1.0), name="users")
items = Relation(block(n_items, n_users + H, 4, 9, n_users + H + n_items, G), zipf(n_items, rows, 1.05), name="items")
n1 = n_users + H + n_items + G
y = rng.normal(0, 1, rows)
rd = RelationalData(y, [users, items], batch_rows=batch_rows)
flat = rd.expand().cache()
L = _ffi.load()
models = {"flat": FMModel(n1 - 1, k, seed=3, init_on_device=True)}
if not flat_only:
    models["relational"] = FMModel(n1 - 1, k, seed=3, init_on_device=True)
    rd.cache()
eta, regw, regv = 0.02, 1e-4, 1e-4


def epoch(name):
    hm = models[name].handle
    _ffi.check(L.fmhip_synchronize(hm))
    t = time.perf_counter()
    if name == "flat":
        _ffi.check(L.fmhip_sgd_epoch(hm, flat.handle, eta, 0.0, regw, regv, None, None))
    else:
        _ffi.check(L.fmhip_relational_sgd_epoch(hm, rd.rel_handle, eta, 0.0, regw, regv, None, None))
    _ffi.check(L.fmhip_synchronize(hm))
    return time.perf_counter() - t


def breakdown(name):
    """HIP-event time per step of the launches the library's profile sees (the flat step: all of them; the relational step: its
    backward, fixup and apply launches — the q-mode forwards, k_rel_finish and k_rel_gather_sum are the rest of its step time)."""
    hm = models[name].handle
    _ffi.check(L.fmhip_profile_begin(hm))
    epoch(name)
    p = _ffi.Profile()
    _ffi.check(L.fmhip_profile_end(hm, C.byref(p)))
    return {kind: v["ms"] / steps * 1e3 for kind, v in p.as_dict().items() if v["launches"]}


steps = flat.n_batches
for name in models:       # warm-up: every kernel instance loaded, tables touched
    epoch(name)
    epoch(name)
times = {name: [] for name in models}
for _ in range(rounds):
    for name in models:
        times[name].append(epoch(name))
walk = 4 * k + 12                                  # bytes a walk moves per stored nonzero (Kp = k = 32)
nnz_blocks = users.block.nnz + items.block.nnz
touched = sum(len(np.unique(rel.mapping[b * batch_rows:(b + 1) * batch_rows])) for rel in (users, items) for b in range(steps)) / steps
rows_b = rows / steps
out = dict(rows=rows, batches=steps, users=n_users, items=n_items, k=k, features=n1, rounds=rounds, nnz_flat_per_batch=flat.nnz / steps,
           nnz_blocks=nnz_blocks, touched_block_rows_per_batch=touched,
           # forward + backward walk every stored nonzero of what they cover once each
           flat_walk_mb=2 * flat.nnz / steps * walk / 1e6,
           # the blocks' two walks; k_rel_finish: 2 q rows read + 1 P row written per data row; k_rel_gather_sum: a P row read per
           # relation and data row, a P_b row written per touched block row (+ the tables' zeroing)
           relational_walk_mb=2 * nnz_blocks * walk / 1e6,
           relational_combine_mb=(rows_b * (3 + 2) + touched + n_users + n_items) * 4 * k / 1e6,
           dense_update_mb=3 * n1 * 4 * k / 1e6)
for name in models:
    t = np.array(times[name]) / steps * 1e3
    out[name] = dict(step_ms_median=float(np.median(t)), step_ms_min=float(t.min()), step_ms_max=float(t.max()), kernels_us=breakdown(name))
if not flat_only:
    out["flat_over_relational"] = out["flat"]["step_ms_median"] / out["relational"]["step_ms_median"]
    out["bytes_flat_over_relational"] = (out["flat_walk_mb"] + out["dense_update_mb"]) / (
        out["relational_walk_mb"] + out["relational_combine_mb"] + out["dense_update_mb"])
print(json.dumps(out))
