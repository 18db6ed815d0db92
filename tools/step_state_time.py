#!/usr/bin/env python3
"""Host time per step of a one-rank touched-rows step loop at a small shape, where the host path IS the cost: every step is a
forward, three backward intervals into the compact buffer, their all-reduces (world 1 over RCCL: nothing of Python inside the loop) and the rows-only
updates as the slices arrive — a dozen short launches the host has to get out.  Run it once per build of the library
(FMHIP_LIB=sparkfm_amd/lib/libfmhip_<name>.so, tools/build_variant.sh), alternating the builds in one job.
    python3 tools/step_state_time.py [k, default 8] [steps per window, default 3000] [windows, default 7]
600 Zipf rows in 3 batches of 200, 300 features, 1 to 12 entries per row, cuts at the shares (0.3, 0.6) of the stored nonzeros.
A window is a host clock around `steps` steps that ends in a device synchronise; one warm-up window first.  Prints the windows'
microseconds per step, their median and their minimum."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparkfm_amd import DataSet, FMModel, _ffi, synth  # noqa: E402
from sparkfm_amd.distributed import HipDataParallelSGD, RcclComm  # noqa: E402

k = int(sys.argv[1]) if len(sys.argv) > 1 else 8
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3000
windows = int(sys.argv[3]) if len(sys.argv) > 3 else 7
N1 = 300
L = _ffi.load()
ds = DataSet.from_arrays(synth.make_zipf(2026, 600, N1, 1, 12, zipf_s=1.05), batch_rows=200).cache()
rng = np.random.default_rng(1000 + k)
fm = FMModel(N1 - 1, k)
fm.w0, fm.w, fm.v = float(rng.normal(0, 0.1)), rng.normal(0, 0.1, N1), rng.normal(0, 0.1, (k, N1))
comm = RcclComm(fm, 0, 1, unique_id=RcclComm.unique_id())
dp = HipDataParallelSGD(comm, eta=1e-3, regw=1e-3, regv=1e-3, exchange="touched", upper_fractions=(0.3, 0.6))
dp.plan(fm, ds)
positions = np.ascontiguousarray(np.arange(steps) % 3, np.int64)
us = []
for w in range(windows + 1):
    _ffi.check(L.fmhip_synchronize(fm.handle))
    t0 = time.perf_counter()
    _ffi.check(L.fmhip_dp_steps(fm.handle, ds.handle, _ffi.ptr(positions), steps, comm.handle, dp.eta, dp.reg0, dp.regw, dp.regv))
    _ffi.check(L.fmhip_synchronize(fm.handle))
    if w:
        us.append((time.perf_counter() - t0) / steps * 1e6)
print("touched-rows step loop k=%d, %d steps per window: us/step %s | median %.2f min %.2f"
      % (k, steps, " ".join("%.2f" % x for x in us), float(np.median(us)), min(us)))
comm.close()
