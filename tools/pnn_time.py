#!/usr/bin/env python
"""Time of the PNN's step (fmhip_pnn_step: forward — the Gram tiles and the MLP, forwards and backwards —, wgrad, the FwFM's backward
and update, dupdate) and of its scoring pass on the two CTR-like shapes of tools/fwfm_time.py, with DeepFM's step at the same hidden
sizes beside it for scale, in one session:

    criteo   39 fields, one entry per field, 2^20 features, batches of 65,536 rows
    avazu    22 fields, the same otherwise

    python tools/pnn_time.py [--shapes criteo,avazu] [--ks 16,4] [--hidden 256-128-64,64-32] [--batches 2] [--rounds 5]
                             [--optimizer adagrad] [--limit 300] [--out FILE]

This process never opens the GPU: per shape it starts one child process under its own time limit (--limit seconds; a child that runs
into it is killed and the tool fails).  The child times the steps with the profiler off, as tools/afm_time.py does (a round is one
epoch inside a host clock that ends in the epoch's statistics read; one warm-up epoch first; median, min and max of --rounds rounds,
per step, in milliseconds): the PNN at every (k, hidden), trained and with the dense part frozen (forward + the FwFM's two launches:
the difference is wgrad + dupdate), its scoring pass per batch (the forward launch's forward half plus the copy to the host), then
DeepFM.  Prints one JSON document."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from fwfm_time import BATCH_ROWS, N_FEATURES, SHAPES, epochs_ms, make  # noqa: E402 — the FwFM profile's shapes and clock


def time_shape(name, fields, ks, hiddens, batches, rounds, optimizer, neighbours):
    import sparkfm_amd as S
    from sparkfm_amd.deepfm import deepfm_init
    from sparkfm_amd.pnn import pnn_init
    row_ptr, col, field, val, y = make(fields, batches * BATCH_ROWS, 20261126)
    out = dict(shape=name, fields=fields, features=N_FEATURES, batch_rows=BATCH_ROWS, batches=batches, nnz_per_batch=len(col) // batches,
               pnn_step_ms={}, pnn_frozen_step_ms={}, pnn_score_ms={}, pnn_logloss_after={}, deepfm_step_ms={})
    ds = S.FFMDataSet.from_arrays(row_ptr, col, field, val, y, batch_rows=BATCH_ROWS).cache()
    rule = dict(loss="logistic", optimizer=optimizer, eta=0.05, regv=2e-5, adagrad_init=1.0)
    zeros = np.zeros(N_FEATURES)
    for k in ks:
        for hidden in hiddens:
            key = "%d/%s" % (k, "-".join(map(str, hidden)))
            m = S.PNNModel(N_FEATURES - 1, fields, k, hidden)
            m.set_params(0.0, zeros, *pnn_init(1, N_FEATURES - 1, fields, k, hidden))
            hip = S.HipPNN.run(**rule)
            out["pnn_step_ms"][key] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
            out["pnn_logloss_after"][key] = m.computeLogLoss(ds)
            frozen = S.HipPNN.run(deep=False, **rule)
            out["pnn_frozen_step_ms"][key] = epochs_ms(lambda: frozen.learn(m, ds), batches, rounds)
            times = []
            for _ in range(rounds + 1):          # the scoring pass over all batches, its copy to the host included; the first is the warm-up
                t0 = time.perf_counter()
                m.predict(ds)
                times.append((time.perf_counter() - t0) * 1e3 / batches)
            out["pnn_score_ms"][key] = dict(median=float(np.median(times[1:])), min=min(times[1:]), max=max(times[1:]))
            m.close()
            if neighbours:
                m = S.DeepFMModel(N_FEATURES - 1, fields, k, hidden)
                m.set_params(0.0, zeros, *deepfm_init(1, N_FEATURES - 1, fields, k, hidden))
                hip = S.HipDeepFM.run(**rule)
                out["deepfm_step_ms"][key] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
                m.close()
    ds.close()
    return out


def child(shape, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", shape, "--batches", str(a.batches), "--rounds", str(a.rounds), "--optimizer", a.optimizer,
           "--ks", a.ks, "--hidden", a.hidden] + (["--alone"] if a.alone else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit)          # (TimeoutExpired kills the child)
    if r.returncode != 0:
        raise SystemExit("pnn_time.py: %r ended with status %d" % (cmd, r.returncode))
    print("pnn_time.py: %s k %s hidden %s done" % (shape, a.ks, a.hidden), file=sys.stderr, flush=True)
    return r.stdout.decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="criteo,avazu")
    ap.add_argument("--ks", default="16,4")
    ap.add_argument("--hidden", default="256-128-64,64-32", help="comma-separated hidden shapes, a shape's widths joined by -")
    ap.add_argument("--batches", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--optimizer", default="adagrad", choices=["sgd", "adagrad"])
    ap.add_argument("--limit", type=int, default=300, help="seconds every child process may take")
    ap.add_argument("--alone", action="store_true", help="the PNN only, without DeepFM")
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("pnn_time.py measures on the GPU: none found")
        hiddens = [tuple(int(n) for n in h.split("-")) for h in a.hidden.split(",")]
        print(json.dumps(time_shape(a.worker, SHAPES[a.worker], [int(k) for k in a.ks.split(",")], hiddens, a.batches, a.rounds, a.optimizer, not a.alone)))
        return
    results = [json.loads(child(shape, a).strip().splitlines()[-1]) for shape in a.shapes.split(",")]
    text = json.dumps(dict(tool="pnn_time", optimizer=a.optimizer, results=results), indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
