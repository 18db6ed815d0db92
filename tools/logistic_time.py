#!/usr/bin/env python3
"""The cost of the logistic loss: fmhip_sgd_epoch with the squared and with the logistic loss, alternated in one process on the
same rows and model (labels binarised at the median, so both losses train on the same data), after a warm-up, each epoch timed to
a device synchronise.  The logistic row finish adds one exp per row to a forward of ~40 gathers per row.
    python3 tools/logistic_time.py [C3|C5] [rows] [rounds]"""
import ctypes as C
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
d["y"] = np.where(d["y"] > np.median(d["y"]), 1.0, 0.0).astype(np.float32)
n1, k = cfg["features"], cfg["k"]
L = _ffi.load()
ds = DataSet.from_arrays(d, batch_rows=cfg.get("batch", 250_000)).cache()
fm = FMModel(n1 - 1, k, seed=3, init_on_device=True)
hm, hd = fm.handle, ds.handle
eta, regw, regv = 0.02, 1e-4, 1e-4


def epoch(loss):
    _ffi.check(L.fmhip_model_set_loss(hm, loss))
    _ffi.check(L.fmhip_synchronize(hm))
    t = time.perf_counter()
    _ffi.check(L.fmhip_sgd_epoch(hm, hd, eta, 0.0, regw, regv, None, None))
    _ffi.check(L.fmhip_synchronize(hm))
    return time.perf_counter() - t


for loss in (_ffi.LOSS_SQUARED, _ffi.LOSS_LOGISTIC):      # warm-up: both kernel instances loaded, tables touched
    epoch(loss)
t_sq, t_lg = [], []
for _ in range(rounds):
    t_sq.append(epoch(_ffi.LOSS_SQUARED))
    t_lg.append(epoch(_ffi.LOSS_LOGISTIC))
st = _ffi.Stats()
r = C.c_double()
_ffi.check(L.fmhip_logloss(hm, hd, C.byref(r), C.byref(st)))
sq, lg = float(np.median(t_sq)), float(np.median(t_lg))
print("%s: %d rows in %d batches, k = %d; fmhip_sgd_epoch median of %d: squared %.2f ms, logistic %.2f ms, logistic / squared %.4f "
      "(min %.2f / %.2f ms); log-loss of the final model (trained under both losses in turn) %.4f" % (cfg_name, rows, ds.n_batches, k, rounds, sq * 1e3, lg * 1e3, lg / sq,
                                                               min(t_sq) * 1e3, min(t_lg) * 1e3, r.value))
