#!/usr/bin/env python
"""Time of AutoInt's step (fmhip_autoint_step) and of its scoring pass on the two CTR-like shapes of tools/fwfm_time.py, with DeepFM's
and the cross network's step on the same rows beside it, in one session:

    criteo   39 fields, one entry per field, 2^20 features, batches of 65,536 rows
    avazu    22 fields, the same otherwise

    python tools/autoint_time.py [--shapes criteo,avazu] [--ks 4,16] [--models 2-2-16,3-2-32] [--batches 4] [--rounds 7] [--limit 300] [--out FILE]

This process never opens the GPU: per shape it starts one child process under its own time limit (--limit seconds; a child that runs
into it is killed and the tool fails).  A round is one epoch (--batches steps, nothing inside it synchronises with the host) inside a
host clock that ends in the epoch's statistics read; one warm-up epoch first; per series the median, min and max of --rounds rounds, per
step, in milliseconds: AutoInt at every (k, L-H-d), trained and with the attention part frozen, its scoring pass per batch (the forward
launch alone, its copy to the host included), then DeepFM (256, 128, 64) and DCN (3, 64) at every k.  `flops` is the forward's work per
pass, rows sum_l (8 F D_l A + 4 F^2 A) with D_0 = k; a training launch does it about three times over.  Prints one JSON document."""
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


def time_shape(name, fields, ks, models, batches, rounds):
    import sparkfm_amd as S
    from sparkfm_amd.autoint import autoint_init
    from sparkfm_amd.dcn import dcn_init
    from sparkfm_amd.deepfm import deepfm_init
    row_ptr, col, field, val, y = make(fields, batches * BATCH_ROWS, 20261126)
    out = dict(shape=name, fields=fields, features=N_FEATURES, batch_rows=BATCH_ROWS, batches=batches, autoint_step_ms={}, autoint_frozen_step_ms={},
               autoint_score_ms={}, flops={}, deepfm_step_ms={}, dcn_step_ms={})
    ds = S.FFMDataSet.from_arrays(row_ptr, col, field, val, y, batch_rows=BATCH_ROWS).cache()
    rule = dict(loss="logistic", optimizer="adagrad", eta=0.2, regv=2e-5, adagrad_init=1.0)
    for k in ks:
        for L, H, d in models:
            key, A = "%d/%d-%d-%d" % (k, L, H, d), H * d
            m = S.AutoIntModel(N_FEATURES - 1, fields, k, L, H, d)
            v, Ws, u = autoint_init(1, N_FEATURES - 1, fields, k, L, H, d)
            m.set_params(0.0, np.zeros(N_FEATURES), v, Ws, u)
            hip = S.HipAutoInt.run(**rule)
            out["autoint_step_ms"][key] = epochs_ms(lambda: hip.learn(m, ds), batches, rounds)
            frozen = S.HipAutoInt.run(attention=False, **rule)
            out["autoint_frozen_step_ms"][key] = epochs_ms(lambda: frozen.learn(m, ds), batches, rounds)
            times = []
            for _ in range(rounds + 1):          # the first is the warm-up
                t0 = time.perf_counter()
                m.predict(ds)
                times.append((time.perf_counter() - t0) * 1e3 / batches)
            out["autoint_score_ms"][key] = dict(median=float(np.median(times[1:])), min=min(times[1:]), max=max(times[1:]))
            out["flops"][key] = BATCH_ROWS * sum(8 * fields * (k if l == 0 else A) * A + 4 * fields * fields * A for l in range(L))
            m.close()
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="criteo,avazu")
    ap.add_argument("--ks", default="4,16")
    ap.add_argument("--models", default="2-2-16,3-2-32", help="comma-separated models, layers-heads-head_dim")
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=300, help="seconds every child process may take")
    ap.add_argument("--worker", help=argparse.SUPPRESS)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.worker:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("autoint_time.py measures on the GPU: none found")
        models = [tuple(int(n) for n in c.split("-")) for c in a.models.split(",")]
        print(json.dumps(time_shape(a.worker, SHAPES[a.worker], [int(k) for k in a.ks.split(",")], models, a.batches, a.rounds)))
        return
    results = []
    for shape in a.shapes.split(","):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", shape, "--batches", str(a.batches), "--rounds", str(a.rounds), "--ks", a.ks,
               "--models", a.models]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=a.limit)          # (TimeoutExpired kills the child)
        if r.returncode != 0:
            raise SystemExit("autoint_time.py: %r ended with status %d" % (cmd, r.returncode))
        results.append(json.loads(r.stdout.decode().strip().splitlines()[-1]))
    text = json.dumps(dict(tool="autoint_time", results=results), indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
