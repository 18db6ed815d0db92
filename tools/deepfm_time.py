#!/usr/bin/env python
"""Time of DeepFM's step (fmhip_deepfm_step) and of its five launches (forward — the MLP forwards and backwards per row tile —, wgrad,
the FwFM's backward and update, dupdate) on the two CTR-like shapes of tools/fwfm_time.py, with the FwFM's and the FmFM's step on the
same rows beside it, in one session:

    criteo   39 fields, one entry per field, 2^20 features, batches of 65,536 rows
    avazu    22 fields, the same otherwise

    python tools/deepfm_time.py [--shapes criteo,avazu] [--ks 4,16] [--hidden 256-128-64,64-32] [--batches 4] [--rounds 7] [--optimizer adagrad]
                                [--limit 300] [--no-trace] [--out FILE]

This process never opens the GPU: per shape it starts a few child processes, each under its own time limit (--limit seconds; a child
that runs into it is killed and the tool fails).  The first times the steps with the profiler off: a round is one epoch (--batches
steps, nothing inside it synchronises with the host) inside a host clock that ends in the epoch's statistics read; one warm-up epoch
first; per series the median, min and max of --rounds rounds, per step, in milliseconds: DeepFM at every (k, hidden), trained and with
the dense part frozen, then the FwFM and the FmFM at every k.  The others, one per (k, hidden), run the same child (2 rounds of 2
batches) under `rocprofv3 --kernel-trace --stats` and read the kernels' mean times per instance from its statistics.  `flops` is the
work of the dense products, computed from the shapes: 2 rows sum_l n_{l-1} n_l with n_0 = F Kp rounded up to 16, once for the layers
forwards, once for delta and J backwards (both in the forward launch), once for the weight gradients.  Prints one JSON document."""
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


def time_shape(name, fields, ks, hiddens, batches, rounds, optimizer, neighbours):
    import sparkfm_amd as S
    from sparkfm_amd.deepfm import deepfm_init
    from sparkfm_amd.fmfm import identity_matrices
    from sparkfm_amd.fwfm import fwfm_init
    n_rows = batches * BATCH_ROWS
    row_ptr, col, field, val, y = make(fields, n_rows, 20261126)
    out = dict(shape=name, fields=fields, features=N_FEATURES, batch_rows=BATCH_ROWS, batches=batches, nnz_per_batch=len(col) // batches,
               deepfm_step_ms={}, deepfm_frozen_step_ms={}, deepfm_logloss_after={}, fwfm_step_ms={}, fmfm_step_ms={}, flops={})
    ds = S.FFMDataSet.from_arrays(row_ptr, col, field, val, y, batch_rows=BATCH_ROWS).cache()
    rule = dict(loss="logistic", optimizer=optimizer, eta=0.2, regv=2e-5, adagrad_init=1.0)
    for k in ks:
        for hidden in hiddens:
            key = "%d/%s" % (k, "-".join(map(str, hidden)))
            m = S.DeepFMModel(N_FEATURES - 1, fields, k, hidden)
            v, layers, u = deepfm_init(1, N_FEATURES - 1, fields, k, hidden)
            m.set_params(0.0, np.zeros(N_FEATURES), v, layers, u)
            hip = S.HipDeepFM.run(**rule)
            out["deepfm_step_ms"][key] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
            out["deepfm_logloss_after"][key] = m.computeLogLoss(ds)
            frozen = S.HipDeepFM.run(deep=False, **rule)
            out["deepfm_frozen_step_ms"][key] = epochs_ms(lambda: frozen.learn(m, ds), batches, rounds)
            widths = ((fields * m.padded_factors + 15) // 16 * 16,) + tuple(hidden)
            out["flops"][key] = dict(widths=widths, per_pass=2 * BATCH_ROWS * sum(a * b for a, b in zip(widths, widths[1:])))
            m.close()
        if not neighbours:
            continue
        v0 = fwfm_init(1, N_FEATURES - 1, k)
        m = S.FwFMModel(N_FEATURES - 1, fields, k)
        m.set_params(0.0, np.zeros(N_FEATURES), v0, np.ones((fields, fields)))
        hip = S.HipFwFM.run(**rule)
        out["fwfm_step_ms"][k] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
        m.close()
        m = S.FmFMModel(N_FEATURES - 1, fields, k)
        m.set_params(0.0, np.zeros(N_FEATURES), v0, identity_matrices(fields, k))
        hip = S.HipFmFM.run(**rule)
        out["fmfm_step_ms"][k] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
        m.close()
    ds.close()
    return out


def child(shape, a, batches, rounds, ks, hidden, neighbours, wrap=()):
    cmd = list(wrap) + [sys.executable, os.path.abspath(__file__), "--worker", shape, "--batches", str(batches), "--rounds", str(rounds),
                        "--optimizer", a.optimizer, "--ks", ks, "--hidden", hidden] + ([] if neighbours else ["--alone"])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit)          # (TimeoutExpired kills the child)
    if r.returncode != 0:
        raise SystemExit("deepfm_time.py: %r ended with status %d" % (cmd, r.returncode))
    print("deepfm_time.py: %s k %s hidden %s%s done" % (shape, ks, hidden, " (traced)" if wrap else ""), file=sys.stderr, flush=True)
    return r.stdout.decode()


def trace(shape, a, k, hidden):
    """The launches' mean times in ms per kernel instance at one (k, hidden), from a kernel trace of a short run of DeepFM alone (its
    trained and its frozen steps share the forward, backward and update instances: theirs are means over both)."""
    with tempfile.TemporaryDirectory() as tmp:
        child(shape, a, 2, 2, k, hidden, False, wrap=["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "t", "--output-format", "csv", "--"])
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                hit = re.search(r"k_(deepfm|fwfm)_\w+(<[^>]*>)?", row["Name"])
                if hit:
                    out[hit.group(0)] = float(row["AverageNs"]) * 1e-6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="criteo,avazu")
    ap.add_argument("--ks", default="4,16")
    ap.add_argument("--hidden", default="256-128-64,64-32", help="comma-separated models, a model's widths joined by '-'")
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--optimizer", default="adagrad", choices=["sgd", "adagrad"])
    ap.add_argument("--limit", type=int, default=300, help="seconds every child process may take")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    ap.add_argument("--alone", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("deepfm_time.py measures on the GPU: none found")
        hiddens = [tuple(int(n) for n in h.split("-")) for h in a.hidden.split(",")]
        print(json.dumps(time_shape(a.worker, SHAPES[a.worker], [int(k) for k in a.ks.split(",")], hiddens, a.batches, a.rounds, a.optimizer, not a.alone)))
        return
    results = []
    for shape in a.shapes.split(","):
        res = json.loads(child(shape, a, a.batches, a.rounds, a.ks, a.hidden, True).strip().splitlines()[-1])
        res["launch_ms"] = None if a.no_trace else {"%s/%s" % (k, h): trace(shape, a, k, h) for k in a.ks.split(",") for h in a.hidden.split(",")}
        results.append(res)
    text = json.dumps(dict(tool="deepfm_time", optimizer=a.optimizer, results=results), indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
