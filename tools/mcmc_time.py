#!/usr/bin/env python
"""Time per epoch of the MCMC learner (fmhip_mcmc_epoch, sampling on) beside the ALS epoch (fmhip_als_epoch), in ONE process and
alternating, on three shapes taken from bench.py by import: BASELINE config 1 (bench.als_c1's: 10,000 x 1,000, k = 8 — the one-wave
LDS walk), a long-column shape of bench.als_long (the chip-wide two-launch step) and bench.als_fields' one-hot two-field shape of 1 M
rows (the level schedule).  Both calls are synchronous (they end with the parameters back on the host), so an epoch is the wall time
of its call.

    python tools/mcmc_time.py [--reps 9] [--shapes c1,long,fields] [--task regression|classification|both] [--parent-lib PATH] [--out FILE]

--task classification / both: the classification epoch (fmhip_mcmc_create_task, the probit link: labels cut at their median, a
truncated-normal draw per row in front of the sweeps) is timed too, as a third series alternating with the other two on a model of
its own.

--parent-lib: another build of libfmhip.so (the parent commit's) — its fmhip_als_epoch is timed in the same process, alternating
parent / this / parent-again / this-again on four models of their own, so that "this against the parent" can be read beside "the
parent against itself".  Every library is driven through the same few raw ctypes bindings (a library without the MCMC symbols binds too).
Prints one JSON document; per series: median, min, max in milliseconds and every sample."""
import argparse
import ctypes as C
import inspect
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bind(path):
    import torch  # noqa: F401  (its HIP runtime first, as sparkfm_amd._ffi does)
    L = C.CDLL(path)
    vp, i32, i64, dbl, P = C.c_void_p, C.c_int32, C.c_int64, C.c_double, C.POINTER
    L.fmhip_last_error.restype = C.c_char_p
    L.fmhip_model_create.argtypes = [C.c_int, i64, i32, vp, P(vp)]
    L.fmhip_model_set_params.argtypes = [vp, dbl, vp, vp]
    L.fmhip_model_destroy.argtypes = [vp]
    L.fmhip_dataset_create.argtypes = [C.c_int, i64, vp, vp, vp, vp, i64, P(vp)]
    L.fmhip_dataset_destroy.argtypes = [vp]
    L.fmhip_als_epoch.argtypes = [vp, vp, dbl, dbl, dbl]
    if hasattr(L, "fmhip_mcmc_create"):
        L.fmhip_mcmc_create.argtypes = [vp, vp, vp, vp, P(vp)]
        L.fmhip_mcmc_epoch.argtypes = [vp, vp]
        L.fmhip_mcmc_destroy.argtypes = [vp]
    if hasattr(L, "fmhip_mcmc_create_task"):
        L.fmhip_mcmc_create_task.argtypes = [vp, vp, vp, vp, vp, P(vp)]
    return L


def ok(L, code):
    if code != 0:
        raise RuntimeError("fmhip error %d: %s" % (code, L.fmhip_last_error().decode("utf-8", "replace")))


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


class TaskOpts(C.Structure):
    _fields_ = [("task", C.c_int32), ("clip", C.c_int32), ("clip_lo", C.c_double), ("clip_hi", C.c_double)]


class Run:
    """One model + its own dataset handle in library L; classification: the MCMC handle is made with the probit task."""

    def __init__(self, L, d, n, k, init, classification=False):
        self.L, self.m, self.d, self.s, self.classification = L, C.c_void_p(), C.c_void_p(), None, classification
        ok(L, L.fmhip_dataset_create(0, len(d["row_ptr"]) - 1, ptr(d["row_ptr"]), ptr(d["col"]), ptr(d["val"]), ptr(d["y"]), 0, C.byref(self.d)))
        ok(L, L.fmhip_model_create(0, n, k, None, C.byref(self.m)))
        ok(L, L.fmhip_model_set_params(self.m, init[0], ptr(init[1]), ptr(init[2])))

    def als(self):
        t = time.perf_counter()
        ok(self.L, self.L.fmhip_als_epoch(self.m, self.d, 0.0, 0.0, 10.0))
        return (time.perf_counter() - t) * 1e3

    def mcmc(self):
        if self.s is None:
            self.s = C.c_void_p()
            if self.classification:
                ok(self.L, self.L.fmhip_mcmc_create_task(self.m, self.d, None, None, C.byref(TaskOpts(1, 0, 0.0, 0.0)), C.byref(self.s)))
            else:
                ok(self.L, self.L.fmhip_mcmc_create(self.m, self.d, None, None, C.byref(self.s)))
        t = time.perf_counter()
        ok(self.L, self.L.fmhip_mcmc_epoch(self.s, None))
        return (time.perf_counter() - t) * 1e3

    def close(self):
        if self.s is not None:
            self.L.fmhip_mcmc_destroy(self.s)
        self.L.fmhip_model_destroy(self.m)
        self.L.fmhip_dataset_destroy(self.d)


def shapes():
    import bench
    from sparkfm_amd import synth
    out = {}
    d = synth.make_config("C1")                                            # bench.als_c1's dataset
    out["c1"] = ("C1: 10000 rows x 1000 features, k=8 (one-wave LDS walk)", d, d["k"])
    n_rows, n_feat, nnz_r = inspect.signature(bench.als_long).parameters["shapes"].default[1]
    k = inspect.signature(bench.als_long).parameters["k"].default
    out["long"] = ("%d rows x %d features, %d per row, k=%d (columns of %d entries: chip-wide step)" % (n_rows, n_feat, nnz_r, k, n_rows * nnz_r // n_feat),
                   lambda: synth.make_zipf(synth.BASE_SEED + 77, n_rows, n_feat, nnz_r, nnz_r, zipf_s=0.0), k)
    fp = inspect.signature(bench.als_fields).parameters
    rows, users, items, kf = (fp[n].default for n in ("n_rows", "users", "items", "k"))

    def fields():
        rng = np.random.default_rng(20261004)                              # bench.als_fields' rows
        pw = 1.0 / (np.arange(items) + 30.0)
        col = np.stack([rng.integers(0, users, rows), users + rng.choice(items, rows, p=pw / pw.sum())], axis=1).reshape(-1).astype(np.int32)
        return dict(row_ptr=np.arange(0, 2 * rows + 1, 2, dtype=np.int64), col=col, val=np.ones(2 * rows), y=rng.integers(1, 6, rows).astype(np.float64))
    out["fields"] = ("%d rows x (%d + %d one-hot ids), k=%d (level schedule)" % (rows, users, items, kf), fields, kf)
    return out


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms)), "samples_ms": [round(x, 4) for x in ms]}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--shapes", default="c1,long,fields")
    ap.add_argument("--task", default="regression", choices=["regression", "classification", "both"])
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from sparkfm_amd import _build
    this = bind(os.environ.get("FMHIP_LIB") or _build.LIB)
    parent = bind(args.parent_lib) if args.parent_lib else None
    table = shapes()
    doc = {"reps": args.reps, "shapes": {}}
    for name in args.shapes.split(","):
        what, d, k = table[name]
        d = d() if callable(d) else d
        d = dict(row_ptr=np.ascontiguousarray(d["row_ptr"], np.int64), col=np.ascontiguousarray(d["col"], np.int32),
                 val=np.ascontiguousarray(d["val"], np.float64), y=np.ascontiguousarray(d["y"], np.float64))
        n = int(d["col"].max())
        init = (0.0, np.zeros(n + 1), np.ascontiguousarray(np.random.default_rng(1).normal(0, 0.01, (n + 1) * k)))
        rec = {"workload": what}
        # ---- MCMC beside ALS, this library, alternating (one warm-up epoch each: allocations)
        a, b = Run(this, d, n, k, init), Run(this, d, n, k, init)
        c = None
        if args.task != "regression":
            cut = dict(d, y=np.ascontiguousarray(d["y"] > np.median(d["y"]), np.float64))
            c = Run(this, cut, n, k, init, classification=True)
            c.mcmc()                                                       # (epoch 0 trains on +-1: every timed epoch draws)
        a.als(), b.mcmc()
        als, mcmc, probit = [], [], []
        for _ in range(args.reps):
            als.append(a.als())
            mcmc.append(b.mcmc())
            if c is not None:
                probit.append(c.mcmc())
        rec["als_epoch"], rec["mcmc_epoch"] = summary(als), summary(mcmc)
        rec["mcmc_over_als"] = rec["mcmc_epoch"]["median_ms"] / rec["als_epoch"]["median_ms"]
        if c is not None:
            rec["mcmc_classification_epoch"] = summary(probit)
            rec["classification_over_regression"] = rec["mcmc_classification_epoch"]["median_ms"] / rec["mcmc_epoch"]["median_ms"]
            c.close()
        b.close()
        # ---- the ALS epoch of this library against the parent's, and the parent's against itself
        if parent is not None:
            # two models of each library, made and timed in turn (parent, this, parent, this): where a model's buffers land moves
            # an epoch by more than the libraries differ, so each library is read from two placements
            a.close()
            runs = [Run(parent, d, n, k, init), Run(this, d, n, k, init), Run(parent, d, n, k, init), Run(this, d, n, k, init)]
            for r in runs:
                r.als()
            ts = [[] for _ in runs]
            for _ in range(args.reps):
                for r, t in zip(runs, ts):
                    t.append(r.als())
            rec["als_parent"], rec["als_this"], rec["als_parent_again"], rec["als_this_again"] = (summary(t) for t in ts)
            med = [rec[n_]["median_ms"] for n_ in ("als_parent", "als_this", "als_parent_again", "als_this_again")]
            rec["this_minus_parent_ms"] = (med[1] + med[3]) / 2 - (med[0] + med[2]) / 2
            rec["parent_again_minus_parent_ms"] = med[2] - med[0]
            rec["this_again_minus_this_ms"] = med[3] - med[1]
            for r in runs:
                r.close()
            a = None
        if a is not None:
            a.close()
        doc["shapes"][name] = rec
        print("# %s: ALS %.3f ms, MCMC %.3f ms%s" % (name, rec["als_epoch"]["median_ms"], rec["mcmc_epoch"]["median_ms"],
                                                   ", classification %.3f ms" % rec["mcmc_classification_epoch"]["median_ms"] if c is not None else ""),
              file=sys.stderr, flush=True)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
