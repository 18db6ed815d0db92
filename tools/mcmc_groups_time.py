#!/usr/bin/env python
"""Time per epoch of the MCMC learner with attribute groups (include/fmhip_mcmc_groups.h) beside the ungrouped handle, in ONE process
and alternating, on tools/mcmc_time.py's three shapes (taken from it by import): ungrouped, G = 2, G = 32 and G = 1024 — feature i
of group i * G / n, contiguous fields — each on a model of its own, one warm-up epoch each.  Every call is synchronous, so an epoch
is the wall time of its call.

    python tools/mcmc_groups_time.py [--reps 9] [--shapes c1,long,fields] [--groups 2,32,1024] [--parent-lib PATH] [--out FILE]

--parent-lib: another build of libfmhip.so (the parent commit's) — its ungrouped fmhip_mcmc_epoch is timed in the same process,
alternating parent / this / parent-again / this-again on four models of their own, as tools/mcmc_time.py does for the ALS epoch.

k_mcmc_group_sums alone: an epoch's wall time cannot show one kernel, so run this tool under the profiler's kernel trace in a run of
its own and read that kernel's row of the statistics (launches, mean, min, max) —
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/mcmc_groups_time.py --reps 3 --shapes fields --groups 32
Prints one JSON document; per series: median, min, max in milliseconds and every sample."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from mcmc_time import Run, bind, ok, ptr, shapes, summary  # noqa: E402


class GroupedRun(Run):
    """A Run whose MCMC handle gets n_groups contiguous attribute groups before its first epoch (0: none — the ungrouped handle)."""

    def __init__(self, L, d, n, k, init, n_groups=0):
        super().__init__(L, d, n, k, init)
        self.n, self.n_groups = n, n_groups

    def mcmc(self):
        if self.s is None:
            self.s = C.c_void_p()
            ok(self.L, self.L.fmhip_mcmc_create(self.m, self.d, None, None, C.byref(self.s)))
            if self.n_groups:
                table = (np.arange(self.n, dtype=np.int64) * self.n_groups // max(self.n, 1)).astype(np.int32)
                ok(self.L, self.L.fmhip_mcmc_set_groups(self.s, ptr(table), self.n, self.n_groups))
        t = time.perf_counter()
        ok(self.L, self.L.fmhip_mcmc_epoch(self.s, None))
        return (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="c1,long,fields")
    ap.add_argument("--groups", default="2,32,1024")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from sparkfm_amd import _build
    this = bind(os.environ.get("FMHIP_LIB") or _build.LIB)
    this.fmhip_mcmc_set_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32]
    parent = bind(args.parent_lib) if args.parent_lib else None
    counts = [int(g) for g in args.groups.split(",") if g]
    table = shapes()
    doc = {"reps": args.reps, "shapes": {}}
    for name in args.shapes.split(","):
        what, d, k = table[name]
        d = d() if callable(d) else d
        d = dict(row_ptr=np.ascontiguousarray(d["row_ptr"], np.int64), col=np.ascontiguousarray(d["col"], np.int32),
                 val=np.ascontiguousarray(d["val"], np.float64), y=np.ascontiguousarray(d["y"], np.float64))
        n = int(d["col"].max())
        init = (0.0, np.zeros(n + 1), np.ascontiguousarray(np.random.default_rng(1).normal(0, 0.01, (n + 1) * k)))
        rec = {"workload": what, "num_attribute": n}
        runs = [GroupedRun(this, d, n, k, init, g) for g in [0] + counts]
        for r in runs:
            r.mcmc()
        ts = [[] for _ in runs]
        for _ in range(args.reps):
            for r, t in zip(runs, ts):
                t.append(r.mcmc())
        for r, t in zip(runs, ts):
            rec["ungrouped" if not r.n_groups else "G=%d" % r.n_groups] = summary(t)
            r.close()
        base = rec["ungrouped"]["median_ms"]
        rec["over_ungrouped"] = {key: rec[key]["median_ms"] / base for key in rec if key.startswith("G=")}
        if parent is not None:
            runs = [GroupedRun(parent, d, n, k, init), GroupedRun(this, d, n, k, init), GroupedRun(parent, d, n, k, init), GroupedRun(this, d, n, k, init)]
            for r in runs:
                r.mcmc()
            ts = [[] for _ in runs]
            for _ in range(args.reps):
                for r, t in zip(runs, ts):
                    t.append(r.mcmc())
            names = ("mcmc_parent", "mcmc_this", "mcmc_parent_again", "mcmc_this_again")
            for key, t in zip(names, ts):
                rec[key] = summary(t)
            med = [rec[key]["median_ms"] for key in names]
            rec["this_minus_parent_ms"] = (med[1] + med[3]) / 2 - (med[0] + med[2]) / 2
            rec["parent_again_minus_parent_ms"] = med[2] - med[0]
            rec["this_again_minus_this_ms"] = med[3] - med[1]
            for r in runs:
                r.close()
        doc["shapes"][name] = rec
        print("# %s: " % name + ", ".join("%s %.3f ms" % (key, rec[key]["median_ms"]) for key in rec if isinstance(rec[key], dict) and "median_ms" in rec[key]),
              file=sys.stderr, flush=True)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
