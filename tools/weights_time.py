#!/usr/bin/env python3
"""The cost of per-row example weights (include/fmhip_weights.h): fmhip_sgd_epoch on the same rows and model with the dataset
unweighted and weighted (weights from {0, 0.25, 1, 3.5}), alternated in one process after a warm-up, each epoch timed to a device
synchronise.  A weighted forward is two launches — the q-mode forward, then k_weight_finish, a stream over P — where the
unweighted one is a single launch; the per-step time of the forward launches (HIP events, fmhip_profile_*) is printed for both,
and the finish launch's byte floor, 2 * rows * Kp * 4 B per batch (P read once, written once).
    python3 tools/weights_time.py [C3|C5] [rows] [rounds] [--plain] [--logistic]
--plain times the unweighted dataset only and touches nothing of the weights' interface: the same script, copied into a
checkout of an earlier commit, times that commit's step on the same data (run the two alternately in one job and compare).
k_weight_finish's own time comes from a kernel trace of this script in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -- python3 tools/weights_time.py C3 1000000 2"""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkfm_amd import DataSet, FMModel, _ffi, synth  # noqa: E402

args = [x for x in sys.argv[1:] if not x.startswith("--")]
plain, logistic = "--plain" in sys.argv, "--logistic" in sys.argv
cfg_name = args[0] if len(args) > 0 else "C3"
rows = int(args[1]) if len(args) > 1 else 1_000_000
rounds = int(args[2]) if len(args) > 2 else 5
cfg = synth.CONFIGS[cfg_name]
d = synth.make_config(cfg_name, rows=rows)
if logistic:
    d["y"] = np.where(d["y"] > np.median(d["y"]), 1.0, 0.0).astype(np.float32)
n1, k = cfg["features"], cfg["k"]
L = _ffi.load()
batch_rows = cfg.get("batch", 250_000)
sets = {"unweighted": DataSet.from_arrays(d, batch_rows=batch_rows).cache()}
if not plain:
    c = np.random.default_rng(11).choice([0.0, 0.25, 1.0, 3.5], size=rows, p=[0.2, 0.3, 0.25, 0.25])
    sets["weighted"] = DataSet.from_arrays(d, batch_rows=batch_rows, weights=c).cache()
fm = FMModel(n1 - 1, k, seed=3, init_on_device=True)
hm = fm.handle
eta, regw, regv = 0.02, 1e-4, 1e-4
_ffi.check(L.fmhip_model_set_loss(hm, _ffi.LOSS_LOGISTIC if logistic else _ffi.LOSS_SQUARED))


def epoch(ds):
    _ffi.check(L.fmhip_synchronize(hm))
    t = time.perf_counter()
    _ffi.check(L.fmhip_sgd_epoch(hm, ds.handle, eta, 0.0, regw, regv, None, None))
    _ffi.check(L.fmhip_synchronize(hm))
    return time.perf_counter() - t


def forward_us(ds):
    """HIP-event time of a step's forward launches (one unweighted, two weighted), mean over an epoch's steps."""
    _ffi.check(L.fmhip_profile_begin(hm))
    _ffi.check(L.fmhip_sgd_epoch(hm, ds.handle, eta, 0.0, regw, regv, None, None))
    p = _ffi.Profile()
    _ffi.check(L.fmhip_profile_end(hm, C.byref(p)))
    f = p.as_dict()["forward"]
    return f["ms"] / max(f["launches"], 1) * 1e3


for ds in sets.values():       # warm-up: every kernel instance loaded, tables touched
    epoch(ds)
    epoch(ds)
times = {name: [] for name in sets}
for _ in range(rounds):
    for name, ds in sets.items():
        times[name].append(epoch(ds))
kp = 32
while kp < k:
    kp *= 2
steps = sets["unweighted"].n_batches
batch = sets["unweighted"].batch_info(0)["rows"]
out = dict(config=cfg_name, rows=rows, batches=steps, k=k, loss="logistic" if logistic else "squared", rounds=rounds,
           finish_floor_mb=2 * batch * kp * 4 / 1e6)
for name, ds in sets.items():
    t = np.array(times[name]) / steps * 1e3
    out[name] = dict(step_ms_median=float(np.median(t)), step_ms_min=float(t.min()), step_ms_max=float(t.max()), forward_us=forward_us(ds))
if not plain:
    out["weighted_over_unweighted"] = out["weighted"]["step_ms_median"] / out["unweighted"]["step_ms_median"]
    out["weighted_rmse"] = fm.computeWeightedRMSE(sets["weighted"])
print(json.dumps(out))
