#!/usr/bin/env python3
"""The BPR trainer's redraw modes (include/fmhip_redraw.h) on the problem of tools/bpr_time.py, tools/bpr_adaptive_time.py and
tools/warp_time.py: a user block (an id feature and 9-29 history features per user), an item block (an id feature and 4-9 genre
features), `interactions` observed (user, item) pairs with Zipf-popular items, n_neg = 1, k = 32.  For every batch size and every
sampler (uniform, the best of 16, WARP at C = 16) one handle and one model per redraw mode; the figure is the wall time of
HipBPR.learn to a device synchronise.

A process holds one build of the library, so every tree measured — this one, and with --parent another checkout of the package
with its own built library (an earlier commit, which knows the per-epoch redraw only) — runs as a child process of its own, the
trees taken turn by turn `repeats` times so that they see the same machine; a child warms up with two epochs per handle and then
times `rounds` rounds, the handles taken turn by turn inside every round.  The figure reported is the median over all rounds of all
of a tree's children.

    python3 tools/redraw_time.py [--parent TREE] [interactions] [users] [items] [batch_pairs,batch_pairs,...] [rounds] [repeats]
    python3 tools/redraw_time.py --leg TREE ... [only]      (a child: one tree, the rounds' times as JSON; `only` = sampler/mode, e.g.
                                                             best_16/batch, keeps that one handle: the leg to run under a profiler)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
leg = parent = None
if args[:1] == ["--leg"]:
    leg, args = args[1], args[2:]
elif args[:1] == ["--parent"]:
    parent, args = args[1], args[2:]
n_inter = int(args[0]) if len(args) > 0 else 1_000_000
n_users = int(args[1]) if len(args) > 1 else 20_000
n_items = int(args[2]) if len(args) > 2 else 5_000
batch_sizes = [int(x) for x in args[3].split(",")] if len(args) > 3 else [250_000, 32_768]
rounds = int(args[4]) if len(args) > 4 else 5
repeats = int(args[5]) if len(args) > 5 else 2
only = args[6] if len(args) > 6 else None
SAMPLERS = {"uniform": dict(n_candidates=1), "best_16": dict(n_candidates=16), "warp_16": dict(n_candidates=16, sampler="warp", margin=1.0)}


def child(tree):
    import numpy as np
    sys.path.insert(0, tree)
    from sparkfm_amd import DataSet, FMModel, HipBPR, _ffi
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
    L = _ffi.load()
    modes = list(getattr(HipBPR, "REDRAWS", ("epoch",)))      # (a tree from before the redraw mode: the per-epoch draw alone)

    def timed(fn, fm):
        _ffi.check(L.fmhip_synchronize(fm.handle))
        t = time.perf_counter()
        fn()
        _ffi.check(L.fmhip_synchronize(fm.handle))
        return time.perf_counter() - t

    out = dict(interactions=int(len(key)), users=n_users, items=n_items, k=k, features=n1, rounds=rounds, modes=modes, runs=[])
    for batch_pairs in batch_sizes:
        names = [(s, m) for s in SAMPLERS for m in modes if only in (None, "%s/%s" % (s, m))]
        bprs, models = {}, {}
        for s, m in names:
            kw = dict(SAMPLERS[s], **({"redraw": m} if m != "epoch" else {}))
            bprs[s, m] = HipBPR.run(users, items, positives, n_neg=1, batch_pairs=batch_pairs, seed=3, eta=0.02, regw=1e-4, regv=1e-4, **kw)
            models[s, m] = FMModel(n1 - 1, k, seed=3, init_on_device=True)
        for n in names:      # warm-up: every kernel instance loaded, workspaces sized, the models away from their initial point
            for _ in range(2):
                bprs[n].learn(models[n])
        epoch_s = {n: [] for n in names}
        for _ in range(rounds):
            for n in names:
                epoch_s[n].append(timed(lambda n=n: bprs[n].learn(models[n]), models[n]))
        out["runs"].append(dict(batch_pairs=bprs[names[0]].batch_pairs, batches=bprs[names[0]].n_batches, pairs=bprs[names[0]].n_pairs,
                                epoch_s={"%s/%s" % n: v for n, v in epoch_s.items()},
                                sample_stats={"%s/%s" % n: bprs[n].sample_stats for n in names}))
        for n in names:
            bprs[n].close()
            models[n].close()
    print("REDRAW_TIME " + json.dumps(out))


def driver():
    import numpy as np
    trees = [("this", ROOT)] + ([("parent", os.path.abspath(parent))] if parent else [])
    legs = {name: [] for name, _ in trees}
    for _ in range(repeats):
        for name, tree in reversed(trees):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", tree] + args, stdout=subprocess.PIPE, check=True)
            line = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("REDRAW_TIME ")][-1]
            legs[name].append(json.loads(line[len("REDRAW_TIME "):]))
    first = legs["this"][0]
    out = dict({key: first[key] for key in ("interactions", "users", "items", "k", "features", "rounds")}, repeats=repeats, runs=[])
    for i, run in enumerate(first["runs"]):
        ms = {}
        for name, _ in trees:
            for key in legs[name][0]["runs"][i]["epoch_s"]:
                v = [x for child_out in legs[name] for x in child_out["runs"][i]["epoch_s"][key]]
                ms["%s/%s" % (name, key)] = dict(median=float(np.median(v)) * 1e3, min=min(v) * 1e3, max=max(v) * 1e3, n=len(v))
        row = dict(batch_pairs=run["batch_pairs"], batches=run["batches"], pairs=run["pairs"], epoch_ms=ms, sample_stats=run["sample_stats"])
        for s in SAMPLERS:
            base = ms.get("parent/%s/epoch" % s, ms["this/%s/epoch" % s])["median"]
            row["%s_over_%s_epoch" % (s, "parent" if parent else "this")] = {
                m: ms["this/%s/%s" % (s, m)]["median"] / base for m in first["modes"]}
        out["runs"].append(row)
    print(json.dumps(out))


if leg:
    child(leg)
else:
    driver()
