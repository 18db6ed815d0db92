#!/usr/bin/env python3
"""Interleaved timing of the forward with and without its raised issue priority (fmhip_tune key FORWARD_KERNEL: 60 with, 61 without; 0 =
the plain kernel, which raises none) in ONE process.

    python tools/fwd_phase_ab.py --phase 61,60 [--config C3] [--batch-rows 250000] [--rounds 6]

Every round walks the values in turn, each over all batches with HIP events around every kernel; prints the median and the
min / max over the rounds of the forward's device time per value, and the backward / fixup medians beside it.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--phase", default="61,60", help="values of FORWARD_KERNEL to alternate")
    ap.add_argument("--config", default="C3")
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--batch-rows", type=int, default=250_000)
    ap.add_argument("--rounds", type=int, default=6)
    args = ap.parse_args()
    from sparkfm_amd import DataSet, FMModel, _ffi, synth
    cfg = synth.CONFIGS[args.config]
    rows = args.rows or min(cfg["rows"], 1_000_000)
    d = synth.make_config(args.config, rows=rows)
    n1, k = cfg["features"], cfg["k"]
    ds = DataSet.from_arrays(d, batch_rows=min(args.batch_rows, rows), device=0).cache()
    fm = FMModel(n1 - 1, k, seed=cfg["seed"] + 1000, device=0, init_on_device=True)
    L = _ffi.load()
    hm, hd, nb = fm.handle, ds.handle, ds.n_batches
    variants = [int(x) for x in args.phase.split(",")]
    res = {v: [] for v in variants}
    for rnd in range(args.rounds + 1):      # round 0 warms up
        for v in variants:
            _ffi.check(L.fmhip_model_tune(hm, _ffi.TUNE_FORWARD_KERNEL, v))
            _ffi.check(L.fmhip_profile_begin(hm))
            for j in range(nb):
                _ffi.check(L.fmhip_sgd_step(hm, hd, j, 0.02, 0.0, 1e-4, 1e-4, None))
            p = _ffi.Profile()
            _ffi.check(L.fmhip_profile_end(hm, C.byref(p)))
            if rnd:
                res[v].append([p.ms[i] / max(p.launches[i], 1) * 1e3 for i in (0, 2, 3)])
    print("config %s rows %d batch %d k %d ablation mask %d" % (args.config, rows, min(args.batch_rows, rows), k, L.fmhip_ablation_mask()))
    print("%-8s %10s %10s %10s %10s %10s" % ("phase", "fwd_med", "fwd_min", "fwd_max", "bwd_med", "fixup_med"))
    for v in variants:
        a = np.array(res[v])
        print("%-8d %10.2f %10.2f %10.2f %10.2f %10.2f" % (v, np.median(a[:, 0]), a[:, 0].min(), a[:, 0].max(), np.median(a[:, 1]), np.median(a[:, 2])))
    st = _ffi.Stats()
    _ffi.check(L.fmhip_step_stats(hm, C.byref(st)))
    print("last batch mse %.9f nonfinite %d" % (st.sse / max(st.rows, 1), st.nonfinite))


if __name__ == "__main__":
    main()
