#!/usr/bin/env python3
"""The cost of FTRL-Proximal (include/fmhip_ftrl.h), measured on the device: fmhip_sgd_epoch under SGD, AdaGrad and FTRL, alternated
in one process on the same rows and model after a warm-up, each epoch timed to a device synchronise and divided by its steps; the
update launch (k_apply / k_apply_rows, HIP events around it: fmhip_profile_*) separated out, with the bytes it must move and the
rate that makes.
    python3 tools/ftrl_time.py C3   [rounds] [--plain]      1 M x 100 k, k = 32, batches of 250 k rows, L2 = 1e-4: every rule's update
                                                            is the DENSE pass over the model (SGD: its merged finish where it applies)
    python3 tools/ftrl_time.py wide [rounds] [--plain]      2^22 features, k = 16 (Kp 32, packed w), batches of 450 k Zipf rows that touch
                                                            about 1.9 M rows of the model, L2 = 1e-4: AdaGrad must rewrite the whole
                                                            model each step, FTRL updates the touched rows only
--plain times SGD and AdaGrad only and touches nothing of FTRL's interface: the same script, copied into a checkout of the parent
commit, times that commit's step on the same data (run the two alternately in one job and compare).
The update's byte floor: per model row Kp floats of V and of G read and written, plus the same of every state table — 4 streams
under SGD, 6 under AdaGrad, 8 under FTRL (dense: all n + 1 rows; rows-only: the batch's touched rows).  --json FILE appends the
figures as one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkfm_amd import DataSet, FMModel, _ffi, synth  # noqa: E402

json_out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
args = [x for x in sys.argv[1:] if not x.startswith("--") and x != json_out]
plain = "--plain" in sys.argv
shape = args[0] if args else "C3"
rounds = int(args[1]) if len(args) > 1 else 5
if shape == "C3":
    cfg = synth.CONFIGS["C3"]
    d = synth.make_config("C3", rows=1_000_000)
    n1, k, batch_rows = cfg["features"], cfg["k"], 250_000
else:
    n1, k, batch_rows = 1 << 22, 16, 450_000
    d = synth.make_zipf(123, 4 * batch_rows, n1, 20, 60, zipf_s=1.05)
    d["y"] = np.where(d["y"] > np.median(d["y"]), 1.0, 0.0).astype(np.float32)
L = _ffi.load()
ds = DataSet.from_arrays(d, batch_rows=batch_rows).cache()
fm = FMModel(n1 - 1, k, seed=3, init_on_device=True)
hm, hd = fm.handle, ds.handle
kp = C.c_int32()
_ffi.check(L.fmhip_model_info(hm, None, None, C.byref(kp)))
Kp = kp.value
eta, l2 = 0.02, 1e-4
_ffi.check(L.fmhip_model_set_loss(hm, _ffi.LOSS_SQUARED if shape == "C3" else _ffi.LOSS_LOGISTIC))
rp = d["row_ptr"]
touched = [len(np.unique(d["col"][rp[b * batch_rows]:rp[min(len(rp) - 1, (b + 1) * batch_rows)]])) for b in range(ds.n_batches)]
STREAMS = {"sgd": 4, "adagrad": 6, "ftrl": 8}


def set_rule(rule):
    if rule == "ftrl":
        _ffi.check(L.fmhip_model_set_ftrl(hm, 1.0, 0.1, 1e-3, 0.0))
    else:
        _ffi.check(L.fmhip_model_set_optimizer(hm, _ffi.optimizer_code(rule), 1e-10, 0.1))


def epoch(rule):
    set_rule(rule)
    _ffi.check(L.fmhip_synchronize(hm))
    t = time.perf_counter()
    _ffi.check(L.fmhip_sgd_epoch(hm, hd, eta, 0.0, l2, l2, None, None))
    _ffi.check(L.fmhip_synchronize(hm))
    return (time.perf_counter() - t) / ds.n_batches


def apply_us(rule):
    """HIP-event time of a step's update launch, mean over an epoch's steps (0 launches: the update ran inside another launch)."""
    set_rule(rule)
    _ffi.check(L.fmhip_profile_begin(hm))
    _ffi.check(L.fmhip_sgd_epoch(hm, hd, eta, 0.0, l2, l2, None, None))
    p = _ffi.Profile()
    _ffi.check(L.fmhip_profile_end(hm, C.byref(p)))
    a = p.as_dict()["apply"]
    return (a["ms"] / a["launches"] * 1e3 if a["launches"] else None), int(a["launches"])


rules = ["sgd", "adagrad"] + ([] if plain else ["ftrl"])
for r in rules:                       # warm-up: every kernel instance loaded, every table touched
    epoch(r)
times = {r: [] for r in rules}
for _ in range(rounds):
    for r in rules:
        times[r].append(epoch(r))
out = dict(shape=shape, plain=plain, rows=len(d["y"]), features=n1, k=k, Kp=Kp, batches=ds.n_batches, batch_rows=batch_rows,
           touched_rows_per_batch=touched, rounds=rounds, rules={})
for r in rules:
    us, launches = apply_us(r)
    # which form the update took is the library's choice; the rows-only one when the batch touches at most half of the model and
    # the rule allows it (SGD: lazy decay; AdaGrad: reg = 0 only; FTRL: always)
    rows_only = shape != "C3" and r != "adagrad" and max(touched) * 2 <= n1
    rows_moved = float(np.mean(touched)) if rows_only else float(n1)
    nbytes = rows_moved * Kp * 4 * STREAMS[r]
    med = float(np.median(times[r]))
    out["rules"][r] = dict(step_ms=med * 1e3, step_ms_min=min(times[r]) * 1e3, step_ms_max=max(times[r]) * 1e3, apply_us=us,
                           apply_launches_per_epoch=launches, apply_share=us * 1e-6 / med if launches else None,
                           apply_bytes=nbytes, apply_gbps=nbytes / (us * 1e-6) / 1e9 if launches else None,
                           update="rows-only" if rows_only else "dense")
    print("%s%s %-7s step %.3f ms (median of %d; min %.3f, max %.3f), update launch %s us x %d per epoch (%s, %.1f MB floor -> %s GB/s, "
          "%s of the step)" % (shape, " [plain]" if plain else "", r, med * 1e3, rounds, min(times[r]) * 1e3, max(times[r]) * 1e3,
                               "%.1f" % us if launches else "n/a", launches,
                               out["rules"][r]["update"], nbytes / 1e6, "%.0f" % out["rules"][r]["apply_gbps"] if launches else "n/a",
                               "%.1f %%" % (100 * out["rules"][r]["apply_share"]) if launches else "n/a"), flush=True)
if json_out:
    with open(json_out, "a") as fh:
        fh.write(json.dumps(out) + "\n")
