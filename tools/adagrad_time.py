#!/usr/bin/env python3
"""The cost of AdaGrad: fmhip_sgd_epoch under SGD and under AdaGrad, alternated in one process on the same rows and model, after
a warm-up, each epoch timed to a device synchronise; once with weight decay (reg > 0: AdaGrad's update is the dense pass over
the whole model, and the SGD step may take its merged finish) and once without (reg = 0: both take the rows-only update where the
batch touches few rows).  Switching the optimizer (re-filling the accumulators) happens outside the timed epochs.
    python3 tools/adagrad_time.py [C3|C5] [rows] [rounds]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkfm_amd import DataSet, FMModel, _ffi, synth  # noqa: E402

cfg_name = sys.argv[1] if len(sys.argv) > 1 else "C3"
rows = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
cfg = synth.CONFIGS[cfg_name]
d = synth.make_config(cfg_name, rows=rows)
n1, k = cfg["features"], cfg["k"]
L = _ffi.load()
ds = DataSet.from_arrays(d, batch_rows=cfg.get("batch", 250_000)).cache()
fm = FMModel(n1 - 1, k, seed=3, init_on_device=True)
hm, hd = fm.handle, ds.handle
eta = 0.02


def epoch(opt, reg):
    _ffi.check(L.fmhip_model_set_optimizer(hm, opt, 1e-10, 0.1))
    _ffi.check(L.fmhip_synchronize(hm))
    t = time.perf_counter()
    _ffi.check(L.fmhip_sgd_epoch(hm, hd, eta, 0.0, reg, reg, None, None))
    _ffi.check(L.fmhip_synchronize(hm))
    return time.perf_counter() - t


for reg, form in ((1e-4, "dense update (reg > 0)"), (0.0, "rows-only update where it pays (reg = 0)")):
    for opt in (_ffi.OPT_SGD, _ffi.OPT_ADAGRAD):             # warm-up: both kernel instances loaded, tables touched
        epoch(opt, reg)
    t_sgd, t_ada = [], []
    for _ in range(rounds):
        t_sgd.append(epoch(_ffi.OPT_SGD, reg))
        t_ada.append(epoch(_ffi.OPT_ADAGRAD, reg))
    s, a = float(np.median(t_sgd)), float(np.median(t_ada))
    print("%s, %s: %d rows in %d batches, k = %d; fmhip_sgd_epoch median of %d: SGD %.2f ms, AdaGrad %.2f ms, AdaGrad / SGD %.4f "
          "(min %.2f / %.2f ms)" % (cfg_name, form, rows, ds.n_batches, k, rounds, s * 1e3, a * 1e3, a / s, min(t_sgd) * 1e3, min(t_ada) * 1e3),
          flush=True)
