#!/usr/bin/env python3
"""The cost of an SGDA step (include/fmhip_sgda.h) beside the steps it is built from, measured on the device: four step forms
alternated in one process on the same rows and model after a warm-up, each timed over an epoch's batches to a device synchronise and
divided by the steps; medians over the rounds.
    (a) fmhip_sgd_step                                  the library's fastest step (its update inside the backward's finish)
    (b) fmhip_step_compute + fmhip_step_apply           the split step: gradient into the packed buffer, the dense update a launch of its own
    (c) fmhip_sgda_step without a validation set        (b) with lambda per group, plus the shadow table's write stream
    (d) fmhip_sgda_step with a validation batch         (c) + a second forward and backward + the two lambda kernels
    python3 tools/sgda_time.py C3     [rounds]      1 M x 100 k, k = 32, batches of 250 k rows; validation: one batch of 250 k rows
    python3 tools/sgda_time.py narrow [rounds]      200 k x 2 k Zipf rows, k = 8 (Kp 32, packed w), batches of 50 k: the model is 256 KB
Ten feature groups of equal width.  --only X runs form X alone (a, b, c or d: for a kernel trace of one form); --json FILE appends
the figures as one JSON line.
The new kernels' byte floors, per model row of Kp floats: k_sgda_apply reads V and G and writes V, the shadow and G (5 streams; k_apply:
4); k_sgda_lambda_partials reads G, V and the shadow and writes G (4 streams); k_sgda_lambda_step reads one partial row per 128 model rows."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkfm_amd import DataSet, FMModel, _ffi, synth  # noqa: E402

json_out = sys.argv[sys.argv.index("--json") + 1] if "--json" in sys.argv else None
only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else None
args = [x for x in sys.argv[1:] if not x.startswith("--") and x not in (json_out, only)]
shape = args[0] if args else "C3"
rounds = int(args[1]) if len(args) > 1 else 7
if shape == "C3":
    cfg = synth.CONFIGS["C3"]
    d = synth.make_config("C3", rows=1_000_000)
    n1, k, batch_rows = cfg["features"], cfg["k"], 250_000
else:
    n1, k, batch_rows = 2000, 8, 50_000
    d = synth.make_zipf(321, 4 * batch_rows, n1, 4, 24, zipf_s=1.05)
L = _ffi.load()
ds = DataSet.from_arrays(d, batch_rows=batch_rows).cache()
rp = d["row_ptr"]
dv = dict(row_ptr=rp[:batch_rows + 1].copy(), col=d["col"][:rp[batch_rows]], val=d["val"][:rp[batch_rows]], y=d["y"][:batch_rows])
val = DataSet.from_arrays(dv, batch_rows=batch_rows).cache()
fm = FMModel(n1 - 1, k, seed=3, init_on_device=True)
hm, hd, hv = fm.handle, ds.handle, val.handle
kp = C.c_int32()
_ffi.check(L.fmhip_model_info(hm, None, None, C.byref(kp)))
Kp = kp.value
G = 10
group = np.ascontiguousarray(np.arange(n1) * G // n1, np.int32)
h = C.c_void_p()
eta, lam = 0.02, 1e-4
_ffi.check(L.fmhip_sgda_create(hm, _ffi.ptr(group), n1, G, lam, lam, C.byref(h)))
nb = ds.n_batches


def form_a(b):
    _ffi.check(L.fmhip_sgd_step(hm, hd, b, eta, 0.0, lam, lam, None))


def form_b(b):
    _ffi.check(L.fmhip_step_compute(hm, hd, b))
    _ffi.check(L.fmhip_step_apply(hm, eta, 0.0, lam, lam))


def form_c(b):
    _ffi.check(L.fmhip_sgda_step(h, hd, b, None, 0, eta, 0.0, 0.0, None, None))


def form_d(b):
    _ffi.check(L.fmhip_sgda_step(h, hd, b, hv, 0, eta, eta, 0.0, None, None))


FORMS = dict(a=form_a, b=form_b, c=form_c, d=form_d)
names = [only] if only else list(FORMS)


def epoch(fn):
    _ffi.check(L.fmhip_synchronize(hm))
    t = time.perf_counter()
    for b in range(nb):
        fn(b)
    _ffi.check(L.fmhip_synchronize(hm))
    return (time.perf_counter() - t) / nb


for name in names:                    # warm-up: every kernel instance loaded, every table touched
    epoch(FORMS[name])
times = {name: [] for name in names}
for _ in range(rounds):
    for name in names:
        times[name].append(epoch(FORMS[name]))
row_bytes = Kp * 4
out = dict(shape=shape, rows=len(d["y"]), features=n1, k=k, Kp=Kp, batches=nb, batch_rows=batch_rows, groups=G, rounds=rounds,
           nnz_per_batch=int(rp[batch_rows]), apply_bytes=5 * n1 * row_bytes, k_apply_bytes=4 * n1 * row_bytes, partials_bytes=4 * n1 * row_bytes,
           step_ms={name: float(np.median(times[name])) * 1e3 for name in names},
           step_ms_min={name: min(times[name]) * 1e3 for name in names}, step_ms_max={name: max(times[name]) * 1e3 for name in names})
for name in names:
    print("%s (%s) step %.3f ms (median of %d; min %.3f, max %.3f)" % (shape, name, out["step_ms"][name], rounds, out["step_ms_min"][name],
                                                                      out["step_ms_max"][name]), flush=True)
if not only:
    m = out["step_ms"]
    print("%s (d)/(a) = %.2f, (c)-(b) = %+.3f ms (the shadow's write stream: %.1f MB), (d)-(c) = %.3f ms (a second forward + backward: "
          "(b) minus its update launch; the lambda kernels read %.1f MB)" % (shape, m["d"] / m["a"], m["c"] - m["b"], n1 * row_bytes / 1e6, m["d"] - m["c"],
                                                                            out["partials_bytes"] / 1e6), flush=True)
_ffi.check(L.fmhip_sgda_destroy(h))
if json_out:
    with open(json_out, "a") as fh:
        fh.write(json.dumps(out) + "\n")
