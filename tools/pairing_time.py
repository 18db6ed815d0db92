#!/usr/bin/env python3
"""The cost of pairwise ranking (fmhip_model_set_pairing): fmhip_sgd_epoch under the logistic loss with pairing off and on,
alternated in one process on the same rows and model (labels binarised at the median), after a warm-up, each epoch timed to a
device synchronise.  A paired forward is two launches — the q-mode forward, then k_pair_finish, a stream over P — where the
unpaired one is a single launch; the per-step time of the forward launches (HIP events, fmhip_profile_*) is printed for both,
and the pair launch's byte floor, 2 * rows * Kp * 4 B per batch (P read once, written once).  k_pair_finish's own time comes
from a kernel trace of this script in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/pairing_time.py C3 1000000 2
    python3 tools/pairing_time.py [C3|C5] [rows] [rounds]"""
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
_ffi.check(L.fmhip_model_set_loss(hm, _ffi.LOSS_LOGISTIC))


def epoch(pairing):
    _ffi.check(L.fmhip_model_set_pairing(hm, pairing))
    _ffi.check(L.fmhip_synchronize(hm))
    t = time.perf_counter()
    _ffi.check(L.fmhip_sgd_epoch(hm, hd, eta, 0.0, regw, regv, None, None))
    _ffi.check(L.fmhip_synchronize(hm))
    return time.perf_counter() - t


def forward_us(pairing):
    """HIP-event time of a step's forward launches (one unpaired, two paired), mean over an epoch's steps."""
    _ffi.check(L.fmhip_model_set_pairing(hm, pairing))
    _ffi.check(L.fmhip_profile_begin(hm))
    _ffi.check(L.fmhip_sgd_epoch(hm, hd, eta, 0.0, regw, regv, None, None))
    p = _ffi.Profile()
    _ffi.check(L.fmhip_profile_end(hm, C.byref(p)))
    f = p.as_dict()["forward"]
    return f["ms"] / max(f["launches"], 1) * 1e3


for pairing in (_ffi.PAIRING_NONE, _ffi.PAIRING_ADJACENT):      # warm-up: every kernel instance loaded, tables touched
    epoch(pairing)
t_off, t_on = [], []
for _ in range(rounds):
    t_off.append(epoch(_ffi.PAIRING_NONE))
    t_on.append(epoch(_ffi.PAIRING_ADJACENT))
f_off, f_on = forward_us(_ffi.PAIRING_NONE), forward_us(_ffi.PAIRING_ADJACENT)
r, c = C.c_double(), C.c_double()
_ffi.check(L.fmhip_pair_logloss(hm, hd, C.byref(r), C.byref(c), None))
kp = 32
while kp < k:
    kp *= 2
batch = ds.batch_info(0)["rows"]
off, on = float(np.median(t_off)), float(np.median(t_on))
print("%s: %d rows in %d batches, k = %d; logistic fmhip_sgd_epoch median of %d: unpaired %.2f ms, paired %.2f ms, paired / unpaired %.4f "
      "(min %.2f / %.2f ms); forward launches per step %.1f us unpaired, %.1f us paired (+%.1f us); k_pair_finish byte floor %.1f MB per "
      "%d-row batch; pair log-loss %.4f, concordance %.4f of the final model (trained both ways in turn)"
      % (cfg_name, rows, ds.n_batches, k, rounds, off * 1e3, on * 1e3, on / off, min(t_off) * 1e3, min(t_on) * 1e3, f_off, f_on, f_on - f_off,
         2 * batch * kp * 4 / 1e6, batch, r.value, c.value))
