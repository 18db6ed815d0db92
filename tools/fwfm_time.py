#!/usr/bin/env python
"""Time of the field-weighted FM's step (fmhip_fwfm_step) and of its three launches (forward, backward, update) on the two CTR-like
shapes of tools/ffm_time.py, with the field-aware FM's step and the plain FM's step on the same rows beside it, in one session:

    criteo   39 fields, one entry per field, 2^20 features, batches of 65,536 rows
    avazu    22 fields, the same otherwise

    python tools/fwfm_time.py [--shapes criteo,avazu] [--ks 4,16,32] [--batches 4] [--rounds 7] [--optimizer adagrad] [--limit 300] [--no-trace] [--out FILE]

This process never opens the GPU: per shape it starts two child processes, each under its own time limit (--limit seconds; a child
that runs into it is killed and the tool fails).  The first times the steps with the profiler off: a round is one epoch (--batches
steps, nothing inside it synchronises with the host) inside a host clock that ends in the epoch's statistics read; one warm-up epoch
first; per series the median, min and max of --rounds rounds, per step, in milliseconds: the FwFM at every k of --ks, then the FFM
(k = 4, as its own profile) and the plain FM (every k).  The second runs the same child (2 rounds of 2 batches) under
`rocprofv3 --kernel-trace --stats` and reads the FwFM kernels' mean times per instance from its statistics (`launch_ms`).  `bytes` is
what each launch must move, computed from the shapes: the forward gathers nnz * Kp * 4 and writes as much (dz) plus blocks * (Fp^2 + Fp)
* 4 of r's partials; the backward reads nnz * Kp * 4 of dz and reads and writes v (and the accumulators) of every column present; the
update reads r's partials.  Prints one JSON document."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"criteo": 39, "avazu": 22}
N_FEATURES, BATCH_ROWS = 1 << 20, 1 << 16


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


def epochs_ms(learn, batches, rounds):
    learn()          # warm-up
    samples = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        learn()
        samples.append((time.perf_counter() - t0) * 1e3 / batches)
    return series(samples)


def time_shape(name, fields, ks, batches, rounds, optimizer):
    import sparkfm_amd as S
    from sparkfm_amd.ffm import libffm_init
    from sparkfm_amd.fwfm import fwfm_init
    n_rows = batches * BATCH_ROWS
    row_ptr, col, field, val, y = make(fields, n_rows, 20261126)
    nnz, fp = len(col) // batches, (fields + 15) // 16 * 16
    cols = int(np.mean([len(np.unique(col[b * nnz:(b + 1) * nnz])) for b in range(batches)]))
    blocks = (BATCH_ROWS + 127) // 128
    out = dict(shape=name, fields=fields, features=N_FEATURES, batch_rows=BATCH_ROWS, batches=batches, nnz_per_batch=nnz, columns_per_batch=cols,
               fwfm_step_ms={}, fm_step_ms={}, fwfm_logloss_after={}, bytes={})
    ds = S.FFMDataSet.from_arrays(row_ptr, col, field, val, y, batch_rows=BATCH_ROWS).cache()
    for k in ks:
        m = S.FwFMModel(N_FEATURES - 1, fields, k)
        m.set_params(0.0, np.zeros(N_FEATURES), fwfm_init(1, N_FEATURES - 1, k), np.ones((fields, fields)))
        hip = S.HipFwFM.run(loss="logistic", optimizer=optimizer, eta=0.2, regv=2e-5, adagrad_init=1.0)
        out["fwfm_step_ms"][k] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
        out["fwfm_logloss_after"][k] = m.computeLogLoss(ds)
        kp, tables = m.padded_factors, 4 if optimizer == "adagrad" else 2
        out["bytes"][k] = dict(forward_gather=nnz * kp * 4, forward_dz=nnz * kp * 4, forward_rpart=blocks * (fp * fp + fp) * 4, backward_dz=nnz * kp * 4,
                               backward_tables=cols * kp * 4 * tables, update_rpart=blocks * (fp * fp + fp) * 4)
        m.close()
    # ---- the field-aware FM on the same rows (k = 4, as profiles/ffm.md)
    m = S.FFMModel(N_FEATURES - 1, fields, 4)
    m.set_params(0.0, np.zeros(N_FEATURES), libffm_init(1, N_FEATURES - 1, fields, 4))
    hip = S.HipFFM.run(loss="logistic", optimizer=optimizer, eta=0.2, regv=2e-5, adagrad_init=1.0)
    out["ffm_step_ms"] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
    m.close()
    ds.close()
    # ---- the plain FM on the same rows
    fds = S.DataSet.from_arrays(dict(row_ptr=row_ptr, col=col, val=val, y=y), batch_rows=BATCH_ROWS, device=0).cache()
    for k in ks:
        fm = S.FMModel(N_FEATURES - 1, k, device=0)
        sgd = S.HipSGD(eta=0.05, reg0=0.0, regw=0.0, regv=0.0, loss="logistic", optimizer=optimizer)
        out["fm_step_ms"][k] = epochs_ms(lambda: sgd.learn(fm, fds), batches, rounds)
        fm.close()
    return out


KERNELS = {"k_fwfm_forward": "forward", "k_fwfm_backward": "backward", "k_fwfm_update": "update"}


def child(shape, a, batches, rounds, wrap=()):
    cmd = list(wrap) + [sys.executable, os.path.abspath(__file__), "--worker", shape, "--batches", str(batches), "--rounds", str(rounds),
                        "--optimizer", a.optimizer, "--ks", a.ks]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit)          # (TimeoutExpired kills the child)
    if r.returncode != 0:
        raise SystemExit("fwfm_time.py: %r ended with status %d" % (cmd, r.returncode))
    return r.stdout.decode()


def trace(shape, a):
    """The FwFM launches' mean times in ms per kernel instance (its template arguments name Kp), from a kernel trace of a short run."""
    with tempfile.TemporaryDirectory() as tmp:
        child(shape, a, 2, 2, wrap=["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "t", "--output-format", "csv", "--"])
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                for key, name in KERNELS.items():
                    if key in row["Name"]:
                        out[re.search(r"k_fwfm_\w+(<[^>]*>)?", row["Name"]).group(0)] = float(row["AverageNs"]) * 1e-6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="criteo,avazu")
    ap.add_argument("--ks", default="4,16,32")
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
            raise SystemExit("fwfm_time.py measures on the GPU: none found")
        print(json.dumps(time_shape(a.worker, SHAPES[a.worker], [int(k) for k in a.ks.split(",")], a.batches, a.rounds, a.optimizer)))
        return
    results = []
    for shape in a.shapes.split(","):
        res = json.loads(child(shape, a, a.batches, a.rounds).strip().splitlines()[-1])
        res["launch_ms"] = None if a.no_trace else trace(shape, a)
        results.append(res)
    text = json.dumps(dict(tool="fwfm_time", optimizer=a.optimizer, results=results), indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
