#!/usr/bin/env python3
"""What an AUC costs: whole calls of fmhip_auc (ungrouped, and with ~10^5 groups), of fmhip_logloss on the same dataset (the same
forward pass: the floor the AUC call adds to) and of the host route (fm.predict, then the twin's formulas in numpy: a sort of the
64-bit words, cumulative sums, uint64 arithmetic), each the median of `rounds` after one warm-up, on a scoring-only dataset.
The host route's integers are compared with the device's while it is at it.
    python3 tools/auc_time.py [C3|C5] [rows] [rounds] [--no-host]
One `rocprofv3 --kernel-trace --stats -- python3 tools/auc_time.py C3 1000000 2 --no-host` splits the call by kernel."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from sparkfm_amd import DataSet, FMModel, _ffi, synth  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
cfg_name = args[0] if len(args) > 0 else "C3"
rows = int(args[1]) if len(args) > 1 else (1_000_000 if cfg_name == "C3" else 1 << 24)
rounds = int(args[2]) if len(args) > 2 else 5
with_host = "--no-host" not in sys.argv
cfg = synth.CONFIGS[cfg_name]
d = synth.make_config(cfg_name, rows=rows)
d["y"] = np.where(d["y"] > np.median(d["y"]), 1.0, 0.0).astype(np.float32)
n1, k = cfg["features"], cfg["k"]
L = _ffi.load()
ds = DataSet.from_arrays(d, scoring=True).cache()
fm = FMModel(n1 - 1, k, seed=3, init_stdev=0.05, init_on_device=True)
hm, hd = fm.handle, ds.handle
groups = np.ascontiguousarray(np.random.default_rng(1).integers(0, 100_000, rows) * 21001 % (2 ** 31), np.int32)


def words_np(yhat, y, g):
    s = yhat.astype(np.float32) + np.float32(0.0)
    u = s.view(np.uint32)
    key = np.where(np.isnan(s), np.uint32(0), np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))).astype(np.uint64)
    w = (key << np.uint64(1)) | (y > 0).astype(np.uint64)
    return w if g is None else w | (g.astype(np.uint64) << np.uint64(33))


def auc_np(yhat, y, g):
    """the formulas of sparkfm_amd/csrc/fm_auc.h, vectorised (uint64 arithmetic wraps as the device's does) -> (u2, pairs, groups, scored)"""
    W = np.sort(words_np(yhat, y, g))
    n = len(W)
    cneg = np.concatenate([[0], np.cumsum(~W & np.uint64(1), dtype=np.uint64)]).astype(np.uint64)
    rstart = np.flatnonzero(np.concatenate([[True], (W[1:] >> np.uint64(1)) != (W[:-1] >> np.uint64(1))]))
    gstart = np.flatnonzero(np.concatenate([[True], (W[1:] >> np.uint64(33)) != (W[:-1] >> np.uint64(33))]))
    rend, gend = np.append(rstart[1:], n), np.append(gstart[1:], n)
    neg_r = cneg[rend] - cneg[rstart]
    pos_r = (rend - rstart).astype(np.uint64) - neg_r
    SA = np.concatenate([[0], np.cumsum(pos_r * (np.uint64(2) * cneg[rstart] + neg_r), dtype=np.uint64)]).astype(np.uint64)
    r0, r1 = np.searchsorted(rstart, gstart), np.append(np.searchsorted(rstart, gstart[1:]), len(rstart))
    neg_g = cneg[gend] - cneg[gstart]
    pos_g = (gend - gstart).astype(np.uint64) - neg_g
    u2_g = SA[r1] - SA[r0] - np.uint64(2) * cneg[gstart] * pos_g
    ok = (pos_g > 0) & (neg_g > 0)
    return int(u2_g[ok].sum(dtype=np.uint64)), int((pos_g * neg_g)[ok].sum(dtype=np.uint64)), len(gstart), int(ok.sum())


def timed(fn):
    _ffi.check(L.fmhip_synchronize(hm))
    t = time.perf_counter()
    out = fn()
    return time.perf_counter() - t, out


def call_auc(g):
    res = _ffi.AucResult()
    _ffi.check(L.fmhip_auc(hm, hd, _ffi.ptr(g), C.byref(res), None))
    return res.as_dict()


def call_logloss():
    r = C.c_double()
    _ffi.check(L.fmhip_logloss(hm, hd, C.byref(r), None))
    return r.value


def call_host(g):
    return auc_np(fm.predict(ds), ds.y, g)


legs = [("fmhip_logloss", call_logloss), ("fmhip_auc", lambda: call_auc(None)), ("fmhip_auc, 1e5 groups", lambda: call_auc(groups))]
if with_host:
    legs += [("host: predict + numpy", lambda: call_host(None)), ("host: predict + numpy, 1e5 groups", lambda: call_host(groups))]
times, last = {}, {}
for name, fn in legs:
    timed(fn)                                       # warm-up
    runs = [timed(fn) for _ in range(rounds)]
    times[name], last[name] = float(np.median([t for t, _ in runs])), runs[-1][1]
print("%s: %d rows, %d entries, k = %d, %d scoring batches; medians of %d" % (cfg_name, rows, len(d["col"]), k, ds.n_batches, rounds))
floor = times["fmhip_logloss"]
for name, _ in legs:
    print("  %-36s %9.2f ms   x%.2f of fmhip_logloss" % (name, times[name] * 1e3, times[name] / floor))
for g, tag in ((None, "fmhip_auc"), (groups, "fmhip_auc, 1e5 groups")):
    r = last[tag]
    print("  %s: auc %.6f gauc %.6f u2 %d pairs %d groups %d scored %d" % (tag, r["auc"], r["gauc"], r["u2"], r["pairs"], r["groups"],
                                                                        r["groups_scored"]))
    host = "host: predict + numpy" + (", 1e5 groups" if g is not None else "")
    if host in last:
        same = last[host] == (r["u2"], r["pairs"], r["groups"], r["groups_scored"])
        print("    the host route's integers %s" % ("agree" if same else "DIFFER: %r" % (last[host],)))
