#!/usr/bin/env python
"""Time of the field-matrixed FM's step (fmhip_fmfm_step) and of its five launches (forward, mgrad, the FwFM's backward and update,
mupdate) on the two CTR-like shapes of tools/fwfm_time.py, with the FwFM's, the field-aware FM's and the plain FM's step on the same
rows beside it, in one session:

    criteo   39 fields, one entry per field, 2^20 features, batches of 65,536 rows
    avazu    22 fields, the same otherwise

    python tools/fmfm_time.py [--shapes criteo,avazu] [--ks 4,16] [--batches 4] [--rounds 7] [--optimizer adagrad] [--limit 300] [--no-trace] [--out FILE]

This process never opens the GPU: per shape it starts a few child processes, each under its own time limit (--limit seconds; a child
that runs into it is killed and the tool fails).  The first times the steps with the profiler off: a round is one epoch (--batches
steps, nothing inside it synchronises with the host) inside a host clock that ends in the epoch's statistics read; one warm-up epoch
first; per series the median, min and max of --rounds rounds, per step, in milliseconds: the FmFM and the FwFM at every k of --ks,
then the FFM (k = 4, as its own profile) and the plain FM (every k).  The others, one per k, run the same child (2 rounds of 2 batches)
under `rocprofv3 --kernel-trace --stats` and read the kernels' mean times per instance from its statistics (`launch_ms[k]`).  `flops` is the
work of the two dense products, computed from the shapes: 2 P^2 rows for Z = S MM in the forward and P^2 rows for the gradient's upper
triangle, P = F Kp.  Prints one JSON document."""
import argparse
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fwfm_time import BATCH_ROWS, N_FEATURES, SHAPES, epochs_ms, make  # noqa: E402 — the FwFM profile's shapes and clock


def time_shape(name, fields, ks, batches, rounds, optimizer):
    import sparkfm_amd as S
    from sparkfm_amd.ffm import libffm_init
    from sparkfm_amd.fmfm import identity_matrices
    from sparkfm_amd.fwfm import fwfm_init
    n_rows = batches * BATCH_ROWS
    row_ptr, col, field, val, y = make(fields, n_rows, 20261126)
    out = dict(shape=name, fields=fields, features=N_FEATURES, batch_rows=BATCH_ROWS, batches=batches, nnz_per_batch=len(col) // batches,
               fmfm_step_ms={}, fmfm_frozen_step_ms={}, fwfm_step_ms={}, fm_step_ms={}, fmfm_logloss_after={}, flops={})
    ds = S.FFMDataSet.from_arrays(row_ptr, col, field, val, y, batch_rows=BATCH_ROWS).cache()
    rule = dict(loss="logistic", optimizer=optimizer, eta=0.2, regv=2e-5, adagrad_init=1.0)
    for k in ks:
        v0 = fwfm_init(1, N_FEATURES - 1, k)
        m = S.FmFMModel(N_FEATURES - 1, fields, k)
        m.set_params(0.0, np.zeros(N_FEATURES), v0, identity_matrices(fields, k))
        hip = S.HipFmFM.run(**rule)
        out["fmfm_step_ms"][k] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
        out["fmfm_logloss_after"][k] = m.computeLogLoss(ds)
        frozen = S.HipFmFM.run(field_matrices=False, **rule)
        out["fmfm_frozen_step_ms"][k] = epochs_ms(lambda: frozen.learn(m, ds), batches, rounds)
        p = fields * m.padded_factors
        out["flops"][k] = dict(P=p, forward=2 * p * p * BATCH_ROWS, mgrad=p * p * BATCH_ROWS)
        m.close()
        m = S.FwFMModel(N_FEATURES - 1, fields, k)
        m.set_params(0.0, np.zeros(N_FEATURES), v0, np.ones((fields, fields)))
        hip = S.HipFwFM.run(**rule)
        out["fwfm_step_ms"][k] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
        m.close()
    # ---- the field-aware FM on the same rows (k = 4, as profiles/ffm.md)
    m = S.FFMModel(N_FEATURES - 1, fields, 4)
    m.set_params(0.0, np.zeros(N_FEATURES), libffm_init(1, N_FEATURES - 1, fields, 4))
    hip = S.HipFFM.run(**rule)
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


def child(shape, a, batches, rounds, ks, wrap=()):
    cmd = list(wrap) + [sys.executable, os.path.abspath(__file__), "--worker", shape, "--batches", str(batches), "--rounds", str(rounds),
                        "--optimizer", a.optimizer, "--ks", ks]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit)          # (TimeoutExpired kills the child)
    if r.returncode != 0:
        raise SystemExit("fmfm_time.py: %r ended with status %d" % (cmd, r.returncode))
    return r.stdout.decode()


def trace(shape, a, k):
    """The launches' mean times in ms per kernel instance at one k (mgrad and mupdate are one instance for every k), from a kernel trace
    of a short run.  The FwFM's backward and update instances serve both models in that run: theirs are means over both."""
    with tempfile.TemporaryDirectory() as tmp:
        child(shape, a, 2, 2, k, wrap=["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "t", "--output-format", "csv", "--"])
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                hit = re.search(r"k_(fmfm|fwfm)_\w+(<[^>]*>)?", row["Name"])
                if hit:
                    out[hit.group(0)] = float(row["AverageNs"]) * 1e-6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="criteo,avazu")
    ap.add_argument("--ks", default="4,16")
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
            raise SystemExit("fmfm_time.py measures on the GPU: none found")
        print(json.dumps(time_shape(a.worker, SHAPES[a.worker], [int(k) for k in a.ks.split(",")], a.batches, a.rounds, a.optimizer)))
        return
    results = []
    for shape in a.shapes.split(","):
        res = json.loads(child(shape, a, a.batches, a.rounds, a.ks).strip().splitlines()[-1])
        res["launch_ms"] = None if a.no_trace else {k: trace(shape, a, k) for k in a.ks.split(",")}
        results.append(res)
    text = json.dumps(dict(tool="fmfm_time", optimizer=a.optimizer, results=results), indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
