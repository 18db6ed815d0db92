#!/usr/bin/env python
"""Time of the CIN's step (fmhip_cin_step) and of its five launches (forward — the layers forwards and backwards per row tile —, wgrad,
the FwFM's backward and update, dupdate) on the two CTR-like shapes of tools/fwfm_time.py, with DeepFM's and DCN's step on the same
rows beside it, in one session:

    criteo   39 fields, one entry per field, 2^20 features, batches of 65,536 rows
    avazu    22 fields, the same otherwise

    python tools/cin_time.py [--shapes criteo,avazu] [--ks 4,16] [--maps 32-32,128-128-128] [--batches 4] [--rounds 7]
                             [--optimizer adagrad] [--limit 300] [--no-trace] [--out FILE]

This process never opens the GPU: per shape it starts a few child processes, each under its own time limit (--limit seconds; a child
that runs into it is killed and the tool fails).  The first times the steps with the profiler off, as tools/dcn_time.py does (a round
is one epoch inside a host clock that ends in the epoch's statistics read; one warm-up epoch first; median, min and max of --rounds
rounds, per step, in milliseconds): the CIN at every (k, maps), trained and with the CIN part frozen, its scoring pass per batch, then
DeepFM (256, 128, 64) and DCN (3, 64) at every k.  The others, one per (k, maps), run the same child (2 rounds of 2 batches) under
`rocprofv3 --kernel-trace --stats` and read the kernels' mean times per instance from its statistics.  `flops` is the work of a layer
product over the batch, 2 rows k sum_l H_{l-1} F H_l: once in the scoring forward and in the wgrad, about three times in the training
forward.  Prints one JSON document."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fwfm_time import BATCH_ROWS, N_FEATURES, SHAPES, epochs_ms, make  # noqa: E402 — the FwFM profile's shapes and clock


def time_shape(name, fields, ks, all_maps, batches, rounds, optimizer, neighbours):
    import sparkfm_amd as S
    from sparkfm_amd.cin import cin_init
    from sparkfm_amd.dcn import dcn_init
    from sparkfm_amd.deepfm import deepfm_init
    row_ptr, col, field, val, y = make(fields, batches * BATCH_ROWS, 20261126)
    out = dict(shape=name, fields=fields, features=N_FEATURES, batch_rows=BATCH_ROWS, batches=batches, nnz_per_batch=len(col) // batches,
               cin_step_ms={}, cin_frozen_step_ms={}, cin_score_ms={}, cin_logloss_after={}, deepfm_step_ms={}, dcn_step_ms={}, flops={})
    ds = S.FFMDataSet.from_arrays(row_ptr, col, field, val, y, batch_rows=BATCH_ROWS).cache()
    rule = dict(loss="logistic", optimizer=optimizer, eta=0.2, regv=2e-5, adagrad_init=1.0)
    for k in ks:
        for maps in all_maps:
            key = "%d/%s" % (k, "-".join(map(str, maps)))
            m = S.CINModel(N_FEATURES - 1, fields, k, maps)
            v, layers, u = cin_init(1, N_FEATURES - 1, fields, k, maps)
            m.set_params(0.0, np.zeros(N_FEATURES), v, layers, u)
            hip = S.HipCIN.run(**rule)
            out["cin_step_ms"][key] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
            out["cin_logloss_after"][key] = m.computeLogLoss(ds)
            frozen = S.HipCIN.run(cin=False, **rule)
            out["cin_frozen_step_ms"][key] = epochs_ms(lambda: frozen.learn(m, ds), batches, rounds)
            times = []
            for _ in range(rounds + 1):          # the scoring pass over all batches, its copy to the host included; the first is the warm-up
                t0 = time.perf_counter()
                m.predict(ds)
                times.append((time.perf_counter() - t0) * 1e3 / batches)
            out["cin_score_ms"][key] = dict(median=float(np.median(times[1:])), min=min(times[1:]), max=max(times[1:]))
            out["flops"][key] = 2 * BATCH_ROWS * k * sum(a * fields * b for a, b in zip((fields,) + tuple(maps[:-1]), maps))
            m.close()
        if not neighbours:
            continue
        m = S.DeepFMModel(N_FEATURES - 1, fields, k, (256, 128, 64))
        v, layers, u = deepfm_init(1, N_FEATURES - 1, fields, k, (256, 128, 64))
        m.set_params(0.0, np.zeros(N_FEATURES), v, layers, u)
        hip = S.HipDeepFM.run(**rule)
        out["deepfm_step_ms"][k] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
        m.close()
        m = S.DCNModel(N_FEATURES - 1, fields, k, 3, 64)
        v, cross, u = dcn_init(1, N_FEATURES - 1, fields, k, 3, 64)
        m.set_params(0.0, np.zeros(N_FEATURES), v, cross, u)
        hip = S.HipDCN.run(**rule)
        out["dcn_step_ms"][k] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
        m.close()
    ds.close()
    return out


def child(shape, a, batches, rounds, ks, maps, neighbours, wrap=()):
    cmd = list(wrap) + [sys.executable, os.path.abspath(__file__), "--worker", shape, "--batches", str(batches), "--rounds", str(rounds),
                        "--optimizer", a.optimizer, "--ks", ks, "--maps", maps] + ([] if neighbours else ["--alone"])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit)          # (TimeoutExpired kills the child)
    if r.returncode != 0:
        raise SystemExit("cin_time.py: %r ended with status %d" % (cmd, r.returncode))
    print("cin_time.py: %s k %s maps %s%s done" % (shape, ks, maps, " (traced)" if wrap else ""), file=sys.stderr, flush=True)
    return r.stdout.decode()


def trace(shape, a, k, maps):
    """The launches' mean times in ms per kernel instance at one (k, maps), from a kernel trace of a short run of the CIN alone."""
    with tempfile.TemporaryDirectory() as tmp:
        child(shape, a, 2, 2, k, maps, False, wrap=["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "t", "--output-format", "csv", "--"])
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                hit = re.search(r"k_(cin|fwfm)_\w+(<[^>]*>)?", row["Name"])
                if hit:
                    out[hit.group(0)] = float(row["AverageNs"]) * 1e-6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="criteo,avazu")
    ap.add_argument("--ks", default="4,16")
    ap.add_argument("--maps", default="32-32,128-128-128", help="comma-separated models, a model's map counts joined by '-'")
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
            raise SystemExit("cin_time.py measures on the GPU: none found")
        all_maps = [tuple(int(n) for n in c.split("-")) for c in a.maps.split(",")]
        print(json.dumps(time_shape(a.worker, SHAPES[a.worker], [int(k) for k in a.ks.split(",")], all_maps, a.batches, a.rounds, a.optimizer, not a.alone)))
        return
    results = []
    for shape in a.shapes.split(","):
        res = json.loads(child(shape, a, a.batches, a.rounds, a.ks, a.maps, True).strip().splitlines()[-1])
        res["launch_ms"] = None if a.no_trace else {"%s/%s" % (k, c): trace(shape, a, k, c) for k in a.ks.split(",") for c in a.maps.split(",")}
        results.append(res)
    text = json.dumps(dict(tool="cin_time", optimizer=a.optimizer, results=results), indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
