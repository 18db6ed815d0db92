#!/usr/bin/env python
"""Time of the field-aware FM's step (fmhip_ffm_step) and of its three launches (forward, backward, update) on two CTR-like shapes,
with the plain FM's step (fmhip_sgd_epoch over the same rows, fields dropped) beside it as context:

    criteo   39 fields, one entry per field, k = 4, 2^20 features, batches of 65,536 rows
    avazu    22 fields, the same otherwise

    python tools/ffm_time.py [--shapes criteo,avazu] [--batches 4] [--rounds 7] [--optimizer adagrad] [--limit 300] [--no-trace] [--out FILE]

This process never opens the GPU: per shape it starts two child processes, each under its own time limit (--limit seconds; a child
that runs into it is killed and the tool fails).  The first times the step with the profiler off: a round is one epoch (--batches
steps, nothing inside it synchronises with the host) inside a host clock that ends in the epoch's statistics read; one warm-up epoch
first; per series the median, min and max of --rounds rounds, per step, in milliseconds; the plain FM follows in the same process.
The second runs the same child (2 rounds of 2 batches) under `rocprofv3 --kernel-trace --stats` and reads the three kernels' mean
times from its statistics (`launch_ms`; tracing slows the host, so the step is not timed there).  Every field owns a slice of the
feature ids and draws from it with a skew.  `bytes` is what each launch must move, computed from the shapes: the forward gathers
nnz * F * Kp * 4 (of every entry's feature row the vectors of the row's fields: all F here), the backward the same count again (per
occurrence its row's partner vectors) and writes a record of F * Kp + 4 floats per column, the update reads those records and reads
and writes V (and the accumulators) of every column present.  Prints one JSON document."""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"criteo": 39, "avazu": 22}
N_FEATURES, BATCH_ROWS, K = 1 << 20, 1 << 16, 4


def make(fields, n_rows, seed):
    rng = np.random.default_rng(seed)
    per = N_FEATURES // fields
    # a field's id: a skewed draw from its own slice (u^3 piles the mass on the slice's first ids)
    local = np.minimum((rng.random((n_rows, fields)) ** 3 * per).astype(np.int64), per - 1)
    col = (local + np.arange(fields)[None, :] * per).astype(np.int32).reshape(-1)
    field = np.tile(np.arange(fields, dtype=np.int32), n_rows)
    val = np.full(n_rows * fields, 1.0 / np.sqrt(fields))          # libffm's unit-norm rows
    y = (rng.random(n_rows) < 0.25).astype(np.float64)
    return np.arange(n_rows + 1, dtype=np.int64) * fields, col, field, val, y


def series(samples):
    return dict(median=float(np.median(samples)), min=float(np.min(samples)), max=float(np.max(samples)), samples=[float(x) for x in samples])


def time_shape(name, fields, batches, rounds, optimizer):
    import sparkfm_amd as S
    from sparkfm_amd.ffm import libffm_init
    n_rows = batches * BATCH_ROWS
    row_ptr, col, field, val, y = make(fields, n_rows, 20261126)
    nnz = len(col)
    out = dict(shape=name, fields=fields, k=K, features=N_FEATURES, batch_rows=BATCH_ROWS, batches=batches, nnz_per_batch=nnz // batches,
               columns_per_batch=int(np.mean([len(np.unique(col[b * BATCH_ROWS * fields:(b + 1) * BATCH_ROWS * fields])) for b in range(batches)])))
    # ---- FFM
    ds = S.FFMDataSet.from_arrays(row_ptr, col, field, val, y, batch_rows=BATCH_ROWS).cache()
    m = S.FFMModel(N_FEATURES - 1, fields, K)
    m.set_params(0.0, np.zeros(N_FEATURES), libffm_init(1, N_FEATURES - 1, fields, K))
    hip = S.HipFFM.run(loss="logistic", optimizer=optimizer, eta=0.2, regv=2e-5, adagrad_init=1.0)
    hip.learn(m, ds)          # warm-up
    samples = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        hip.learn(m, ds)
        samples.append((time.perf_counter() - t0) * 1e3 / batches)
    out["ffm_step_ms"] = series(samples)
    out["ffm_logloss_after"] = m.computeLogLoss(ds)
    kp = m.padded_factors
    out["bytes"] = dict(forward_gather=nnz // batches * fields * kp * 4, backward_gather=nnz // batches * fields * kp * 4,
                        backward_partials=out["columns_per_batch"] * (fields * kp + 4) * 4,
                        update=out["columns_per_batch"] * ((fields * kp + 4) * 4 + fields * kp * 4 * (4 if optimizer == "adagrad" else 2)))
    m.close()
    ds.close()
    # ---- the plain FM on the same rows, as context
    fds = S.DataSet.from_arrays(dict(row_ptr=row_ptr, col=col, val=val, y=y), batch_rows=BATCH_ROWS, device=0).cache()
    fm = S.FMModel(N_FEATURES - 1, K, device=0)
    sgd = S.HipSGD(eta=0.05, reg0=0.0, regw=0.0, regv=0.0, loss="logistic", optimizer=optimizer)
    fm = sgd.learn(fm, fds)
    samples = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fm = sgd.learn(fm, fds)
        samples.append((time.perf_counter() - t0) * 1e3 / batches)
    out["fm_step_ms"] = series(samples)
    return out


KERNELS = {"k_ffm_forward<true>": "forward", "k_ffm_backward": "backward", "k_ffm_update": "update"}


def child(shape, a, batches, rounds, wrap=()):
    cmd = list(wrap) + [sys.executable, os.path.abspath(__file__), "--worker", shape, "--batches", str(batches), "--rounds", str(rounds),
                        "--optimizer", a.optimizer]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit)          # (TimeoutExpired kills the child)
    if r.returncode != 0:
        raise SystemExit("ffm_time.py: %r ended with status %d" % (cmd, r.returncode))
    return r.stdout.decode()


def trace(shape, a):
    """The three launches' mean times in ms, from a kernel trace of a short run of the worker."""
    with tempfile.TemporaryDirectory() as tmp:
        child(shape, a, 2, 2, wrap=["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "t", "--output-format", "csv", "--"])
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for key, name in KERNELS.items():
                    if key in row["Name"]:
                        out[name] = float(row["AverageNs"]) * 1e-6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="criteo,avazu")
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--optimizer", default="adagrad", choices=["sgd", "adagrad"])
    ap.add_argument("--limit", type=int, default=300, help="seconds every child process may take")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("ffm_time.py measures on the GPU: none found")
        print(json.dumps(time_shape(a.worker, SHAPES[a.worker], a.batches, a.rounds, a.optimizer)))
        return
    results = []
    for shape in a.shapes.split(","):
        res = json.loads(child(shape, a, a.batches, a.rounds).strip().splitlines()[-1])
        res["launch_ms"] = None if a.no_trace else trace(shape, a)
        results.append(res)
    text = json.dumps(dict(tool="ffm_time", optimizer=a.optimizer, results=results), indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
