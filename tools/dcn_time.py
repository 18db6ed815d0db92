#!/usr/bin/env python
"""Time of the cross network's step (fmhip_dcn_step) and of its five launches (forward — the cross layers forwards and backwards per
row tile —, wgrad, the FwFM's backward and update, dupdate) on the two CTR-like shapes of tools/fwfm_time.py, with DeepFM's and the
FmFM's step on the same rows beside it, in one session:

    criteo   39 fields, one entry per field, 2^20 features, batches of 65,536 rows
    avazu    22 fields, the same otherwise

    python tools/dcn_time.py [--shapes criteo,avazu] [--ks 4,16] [--cross 3-64,2-256] [--hidden 64-32,256-128-64] [--batches 4] [--rounds 7]
                             [--optimizer adagrad] [--limit 300] [--no-trace] [--out FILE]

This process never opens the GPU: per shape it starts a few child processes, each under its own time limit (--limit seconds; a child
that runs into it is killed and the tool fails).  The first times the steps with the profiler off: a round is one epoch (--batches
steps, nothing inside it synchronises with the host) inside a host clock that ends in the epoch's statistics read; one warm-up epoch
first; per series the median, min and max of --rounds rounds, per step, in milliseconds: the cross network at every (k, L-r), trained
and with the cross part frozen, its scoring pass per batch, then DeepFM at every (k, hidden) and the FmFM at every k.  The others, one
per (k, L-r), run the same child (2 rounds of 2 batches) under `rocprofv3 --kernel-trace --stats` and read the kernels' mean times per
instance from its statistics.  `flops` is the work of the forward launch's products, computed from the shapes: 2 rows L 2 Pp r once
forwards (scoring), twice when training; `tile` is the row tile, LDS bytes and workspace bytes of csrc/fm_dcn.h's formulas at
gfx950's 160 KB of LDS a workgroup.  Prints one JSON document."""
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

LDS_LIMIT = 160 * 1024


def tile(Pp, r, L, rows):
    """csrc/fm_dcn.h: dcn_forward_lds + dcn_forward_static, dcn_row_tile, and the workspace's bytes."""
    lds = {rt: (rt * (2 * (Pp + 4) + r + 4 + 2) + rt + 1 + 3) // 4 * 16 + rt * 24 for rt in (64, 32, 16)}
    rt = next(rt for rt in (64, 32, 16) if lds[rt] <= LDS_LIMIT)
    total = L * (2 * Pp * r + Pp) + Pp
    return dict(row_tile=rt, lds_bytes=lds[rt], workspace_bytes=4 * (rows * (L * (3 * Pp + 2 * r) + (2 if L > 1 else 1) * Pp) + -(-rows // 512) * total))


def time_shape(name, fields, ks, crosses, hiddens, batches, rounds, optimizer, neighbours):
    import sparkfm_amd as S
    from sparkfm_amd.dcn import dcn_init
    from sparkfm_amd.deepfm import deepfm_init
    from sparkfm_amd.fmfm import identity_matrices
    from sparkfm_amd.fwfm import fwfm_init
    n_rows = batches * BATCH_ROWS
    row_ptr, col, field, val, y = make(fields, n_rows, 20261126)
    out = dict(shape=name, fields=fields, features=N_FEATURES, batch_rows=BATCH_ROWS, batches=batches, nnz_per_batch=len(col) // batches,
               dcn_step_ms={}, dcn_frozen_step_ms={}, dcn_score_ms={}, dcn_logloss_after={}, deepfm_step_ms={}, fmfm_step_ms={}, flops={}, tile={})
    ds = S.FFMDataSet.from_arrays(row_ptr, col, field, val, y, batch_rows=BATCH_ROWS).cache()
    rule = dict(loss="logistic", optimizer=optimizer, eta=0.2, regv=2e-5, adagrad_init=1.0)
    for k in ks:
        for L, r in crosses:
            key = "%d/%d-%d" % (k, L, r)
            m = S.DCNModel(N_FEATURES - 1, fields, k, L, r)
            v, cross, u = dcn_init(1, N_FEATURES - 1, fields, k, L, r)
            m.set_params(0.0, np.zeros(N_FEATURES), v, cross, u)
            hip = S.HipDCN.run(**rule)
            out["dcn_step_ms"][key] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
            out["dcn_logloss_after"][key] = m.computeLogLoss(ds)
            frozen = S.HipDCN.run(cross=False, **rule)
            out["dcn_frozen_step_ms"][key] = epochs_ms(lambda: frozen.learn(m, ds), batches, rounds)
            times = []
            for _ in range(rounds + 1):          # the scoring pass over all batches, its copy to the host included; the first is the warm-up
                t0 = time.perf_counter()
                m.predict(ds)
                times.append((time.perf_counter() - t0) * 1e3 / batches)
            out["dcn_score_ms"][key] = dict(median=float(np.median(times[1:])), min=min(times[1:]), max=max(times[1:]))
            Pp = (fields * m.padded_factors + 15) // 16 * 16
            out["flops"][key] = dict(Pp=Pp, scoring=2 * BATCH_ROWS * L * 2 * Pp * r, training=4 * BATCH_ROWS * L * 2 * Pp * r)
            out["tile"][key] = tile(Pp, r, L, BATCH_ROWS)
            m.close()
        if not neighbours:
            continue
        for hidden in hiddens:
            m = S.DeepFMModel(N_FEATURES - 1, fields, k, hidden)
            v, layers, u = deepfm_init(1, N_FEATURES - 1, fields, k, hidden)
            m.set_params(0.0, np.zeros(N_FEATURES), v, layers, u)
            hip = S.HipDeepFM.run(**rule)
            out["deepfm_step_ms"]["%d/%s" % (k, "-".join(map(str, hidden)))] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
            m.close()
        m = S.FmFMModel(N_FEATURES - 1, fields, k)
        m.set_params(0.0, np.zeros(N_FEATURES), fwfm_init(1, N_FEATURES - 1, k), identity_matrices(fields, k))
        hip = S.HipFmFM.run(**rule)
        out["fmfm_step_ms"][k] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
        m.close()
    ds.close()
    return out


def child(shape, a, batches, rounds, ks, cross, neighbours, wrap=()):
    cmd = list(wrap) + [sys.executable, os.path.abspath(__file__), "--worker", shape, "--batches", str(batches), "--rounds", str(rounds),
                        "--optimizer", a.optimizer, "--ks", ks, "--cross", cross, "--hidden", a.hidden] + ([] if neighbours else ["--alone"])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit)          # (TimeoutExpired kills the child)
    if r.returncode != 0:
        raise SystemExit("dcn_time.py: %r ended with status %d" % (cmd, r.returncode))
    print("dcn_time.py: %s k %s cross %s%s done" % (shape, ks, cross, " (traced)" if wrap else ""), file=sys.stderr, flush=True)
    return r.stdout.decode()


def trace(shape, a, k, cross):
    """The launches' mean times in ms per kernel instance at one (k, L-r), from a kernel trace of a short run of the cross network alone
    (its trained and frozen steps and its scoring pass share the FwFM's instances; the forward's scoring instance is its own)."""
    with tempfile.TemporaryDirectory() as tmp:
        child(shape, a, 2, 2, k, cross, False, wrap=["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "t", "--output-format", "csv", "--"])
        out = {}
        for path in glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                hit = re.search(r"k_(dcn|fwfm)_\w+(<[^>]*>)?", row["Name"])
                if hit:
                    out[hit.group(0)] = float(row["AverageNs"]) * 1e-6
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="criteo,avazu")
    ap.add_argument("--ks", default="4,16")
    ap.add_argument("--cross", default="3-64,2-256", help="comma-separated models, layers-rank")
    ap.add_argument("--hidden", default="64-32,256-128-64", help="DeepFM's models beside it, a model's widths joined by '-'")
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
            raise SystemExit("dcn_time.py measures on the GPU: none found")
        crosses = [tuple(int(n) for n in c.split("-")) for c in a.cross.split(",")]
        hiddens = [tuple(int(n) for n in h.split("-")) for h in a.hidden.split(",")]
        print(json.dumps(time_shape(a.worker, SHAPES[a.worker], [int(k) for k in a.ks.split(",")], crosses, hiddens, a.batches, a.rounds, a.optimizer,
                                    not a.alone)))
        return
    results = []
    for shape in a.shapes.split(","):
        res = json.loads(child(shape, a, a.batches, a.rounds, a.ks, a.cross, True).strip().splitlines()[-1])
        res["launch_ms"] = None if a.no_trace else {"%s/%s" % (k, c): trace(shape, a, k, c) for k in a.ks.split(",") for c in a.cross.split(",")}
        results.append(res)
    text = json.dumps(dict(tool="dcn_time", optimizer=a.optimizer, results=results), indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
