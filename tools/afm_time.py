#!/usr/bin/env python
"""Time of the AFM's step (fmhip_afm_step: forward — a wave per row, forwards and backwards —, the FwFM's backward and update, dupdate)
and of its scoring pass on the two CTR-like shapes of tools/fwfm_time.py, with AutoInt's and the CIN's step on the same rows beside
it, in one session:

    criteo   39 fields, one entry per field, 2^20 features, batches of 65,536 rows
    avazu    22 fields, the same otherwise

    python tools/afm_time.py [--shapes criteo,avazu] [--ks 16] [--attention 32,64] [--batches 4] [--rounds 7]
                             [--optimizer adagrad] [--limit 300] [--out FILE]

This process never opens the GPU: per shape it starts one child process under its own time limit (--limit seconds; a child that runs
into it is killed and the tool fails).  The child times the steps with the profiler off, as tools/cin_time.py does (a round is one
epoch inside a host clock that ends in the epoch's statistics read; one warm-up epoch first; median, min and max of --rounds rounds,
per step, in milliseconds): the AFM at every (k, t), trained and with the attention part frozen, its scoring pass per batch, then
AutoInt (2 layers, 2 heads of 16) and the CIN (32, 32) at every k.  `tiles` is the (field, 16-block) tiles a row walks, three times
when training.  Prints one JSON document."""
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


def time_shape(name, fields, ks, ts, batches, rounds, optimizer, neighbours):
    import sparkfm_amd as S
    from sparkfm_amd.afm import afm_init
    from sparkfm_amd.autoint import autoint_init
    from sparkfm_amd.cin import cin_init
    row_ptr, col, field, val, y = make(fields, batches * BATCH_ROWS, 20261126)
    out = dict(shape=name, fields=fields, features=N_FEATURES, batch_rows=BATCH_ROWS, batches=batches, nnz_per_batch=len(col) // batches,
               tiles=sum((fields - 1) // 16 - (i + 1) // 16 + 1 for i in range(fields - 1)),
               afm_step_ms={}, afm_frozen_step_ms={}, afm_score_ms={}, afm_logloss_after={}, autoint_step_ms={}, cin_step_ms={})
    ds = S.FFMDataSet.from_arrays(row_ptr, col, field, val, y, batch_rows=BATCH_ROWS).cache()
    rule = dict(loss="logistic", optimizer=optimizer, eta=0.2, regv=2e-5, adagrad_init=1.0)
    zeros = np.zeros(N_FEATURES)
    for k in ks:
        for t in ts:
            key = "%d/%d" % (k, t)
            m = S.AFMModel(N_FEATURES - 1, fields, k, t)
            m.set_params(0.0, zeros, *afm_init(1, N_FEATURES - 1, k, t))
            hip = S.HipAFM.run(**rule)
            out["afm_step_ms"][key] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
            out["afm_logloss_after"][key] = m.computeLogLoss(ds)
            frozen = S.HipAFM.run(attention=False, **rule)
            out["afm_frozen_step_ms"][key] = epochs_ms(lambda: frozen.learn(m, ds), batches, rounds)
            times = []
            for _ in range(rounds + 1):          # the scoring pass over all batches, its copy to the host included; the first is the warm-up
                t0 = time.perf_counter()
                m.predict(ds)
                times.append((time.perf_counter() - t0) * 1e3 / batches)
            out["afm_score_ms"][key] = dict(median=float(np.median(times[1:])), min=min(times[1:]), max=max(times[1:]))
            m.close()
        if not neighbours:
            continue
        m = S.AutoIntModel(N_FEATURES - 1, fields, k, 2, 2, 16)
        m.set_params(0.0, zeros, *autoint_init(1, N_FEATURES - 1, fields, k, 2, 2, 16))
        hip = S.HipAutoInt.run(**rule)
        out["autoint_step_ms"][k] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
        m.close()
        m = S.CINModel(N_FEATURES - 1, fields, k, (32, 32))
        m.set_params(0.0, zeros, *cin_init(1, N_FEATURES - 1, fields, k, (32, 32)))
        hip = S.HipCIN.run(**rule)
        out["cin_step_ms"][k] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
        m.close()
    ds.close()
    return out


def child(shape, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", shape, "--batches", str(a.batches), "--rounds", str(a.rounds), "--optimizer", a.optimizer,
           "--ks", a.ks, "--attention", a.attention] + (["--alone"] if a.alone else [])
    r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit)          # (TimeoutExpired kills the child)
    if r.returncode != 0:
        raise SystemExit("afm_time.py: %r ended with status %d" % (cmd, r.returncode))
    print("afm_time.py: %s k %s t %s done" % (shape, a.ks, a.attention), file=sys.stderr, flush=True)
    return r.stdout.decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="criteo,avazu")
    ap.add_argument("--ks", default="16")
    ap.add_argument("--attention", default="32,64", help="comma-separated attention factors")
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--optimizer", default="adagrad", choices=["sgd", "adagrad"])
    ap.add_argument("--limit", type=int, default=300, help="seconds every child process may take")
    ap.add_argument("--alone", action="store_true", help="the AFM only, without AutoInt and the CIN")
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("afm_time.py measures on the GPU: none found")
        print(json.dumps(time_shape(a.worker, SHAPES[a.worker], [int(k) for k in a.ks.split(",")], [int(t) for t in a.attention.split(",")], a.batches,
                                    a.rounds, a.optimizer, not a.alone)))
        return
    results = [json.loads(child(shape, a).strip().splitlines()[-1]) for shape in a.shapes.split(",")]
    text = json.dumps(dict(tool="afm_time", optimizer=a.optimizer, results=results), indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
