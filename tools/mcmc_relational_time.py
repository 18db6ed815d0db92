#!/usr/bin/env python
"""Time per epoch of the MCMC learner swept BY BLOCKS over a RelationalData (fmhip_mcmc_create_relational) beside the flat learner on
expand() (fmhip_mcmc_create), in ONE process and alternating, both sampling with the same seed.  Both calls are synchronous (they end
with the parameters back on the host), so an epoch is the wall time of its call.

    python tools/mcmc_relational_time.py [rows users items] [--k 8] [--reps 5] [--history 16384] [--only relational|flat] [--out FILE]

The data is tools/relational_time.py's recommender (profiles/relational.md): a user block (an id feature and 19-59 history features
of `--history` ids), an item block (an id and 4-9 of 64 genres), Zipf mappings, no plain part; defaults 500000 100000 20000.
--only: one of the two series alone — what a `rocprofv3 --kernel-trace --stats -- python tools/mcmc_relational_time.py ... --only
relational` run breaks down by launch.  Prints one JSON document: the entries each sweep walks per parameter group, the columns (one
dependent step each), the walk each part takes, and per series median / min / max in milliseconds with every sample."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def block(rng, n, id0, lo, hi, f0, span):
    """n rows: the id feature id0 + j (value 1), then lo..hi distinct features of [f0, f0 + span) (span a power of two: an odd
    stride from a random start never repeats), value 1 / sqrt(their count) — tools/relational_time.py's."""
    cnt = rng.integers(lo, hi + 1, n)
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(cnt + 1, out=ptr[1:])
    within = np.arange(ptr[-1], dtype=np.int64) - np.repeat(ptr[:-1], cnt + 1)
    start, stride = np.repeat(rng.integers(0, span, n), cnt + 1), np.repeat(rng.integers(0, span // 2, n) * 2 + 1, cnt + 1)
    col = np.where(within == 0, id0 + np.repeat(np.arange(n), cnt + 1), f0 + (start + (within - 1) * stride) % span).astype(np.int32)
    val = np.where(within == 0, 1.0, 1.0 / np.sqrt(np.repeat(cnt, cnt + 1)))
    return ptr, col, val


def zipf(rng, n, size, s):
    p = 1.0 / np.arange(1, n + 1) ** s
    return rng.permutation(n)[rng.choice(n, size=size, p=p / p.sum())].astype(np.int32)


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "samples_ms": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("shape", nargs="*", type=int, default=[500_000, 100_000, 20_000])
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--history", type=int, default=16384)
    ap.add_argument("--only", default=None, choices=["relational", "flat"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows, n_users, n_items = args.shape
    from sparkfm_amd import FMModel, HipBlockMCMC, HipMCMC, Relation, RelationalData
    rng = np.random.default_rng(17)
    H, G, k = args.history, 64, args.k
    users = Relation(block(rng, n_users, 0, 19, 59, n_users, H), zipf(rng, n_users, rows, 1.0), name="users")
    items = Relation(block(rng, n_items, n_users + H, 4, 9, n_users + H + n_items, G), zipf(rng, n_items, rows, 1.05), name="items")
    n1 = n_users + H + n_items + G
    rd = RelationalData(rng.normal(0, 1, rows), [users, items])
    series = {}
    if args.only != "flat":
        series["relational"] = (rd.cache(), FMModel(n1 - 1, k, seed=3), HipBlockMCMC.run(seed=5))
    flat = None
    if args.only != "relational":
        flat = rd.expand().cache()
        series["flat"] = (flat, FMModel(n1 - 1, k, seed=3), HipMCMC.run(seed=5))
    block_nnz = int(users.block.nnz + items.block.nnz)
    flat_nnz = int(sum(np.diff(rel.block.row_ptr)[rel.mapping].sum() for rel in (users, items)))
    doc = {"workload": "%d rows, %d users (%d history ids), %d items, k=%d" % (rows, n_users, H, n_items, k), "reps": args.reps,
           "entries_per_group": {"flat": flat_nnz, "blocks": block_nnz, "blocks_plus_rows_times_parts": block_nnz + 2 * rows},
           "columns": {"users": int(len(np.unique(users.block.col))), "items": int(len(np.unique(items.block.col)))}}
    for name, (ds, fm, mcmc) in series.items():
        t = time.perf_counter()
        mcmc.learn(fm, ds)                                             # warm-up: the handle, the allocations
        doc[name + "_first_epoch_ms"] = (time.perf_counter() - t) * 1e3
    samples = {name: [] for name in series}
    for _ in range(args.reps):
        for name, (ds, fm, mcmc) in series.items():                   # alternating
            t = time.perf_counter()
            mcmc.learn(fm, ds)
            samples[name].append((time.perf_counter() - t) * 1e3)
    for name, ms in samples.items():
        doc[name + "_epoch"] = summary(ms)
        print("# %s: %.1f ms" % (name, doc[name + "_epoch"]["median_ms"]), file=sys.stderr, flush=True)
    if len(samples) == 2:
        doc["flat_over_relational"] = doc["flat_epoch"]["median_ms"] / doc["relational_epoch"]["median_ms"]
        a, b = series["relational"][1], series["flat"][1]
        doc["max_abs_difference_w"] = float(np.abs(a.w - b.w).max())
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")
    for _, _, mcmc in series.values():
        mcmc.close()


if __name__ == "__main__":
    main()
