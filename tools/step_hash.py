#!/usr/bin/env python3
"""Prints hashes of what every ROUTE of a mini-batch step computes — the routes differ in how the pieces of a step (forward,
backward intervals, exchange, update) hand the step's state to each other (StepState, sparkfm_amd/csrc/fmhip_internal.h), not
in their kernels — on fixed small data: run it with two builds of the library (FMHIP_LIB=sparkfm_amd/lib/libfmhip_<name>.so,
tools/build_variant.sh) to check that a change to the host side of the step left every bit where it was.  tools/finish_hash.py
does the same for the finishes behind a q-mode forward, tools/grad_hash.py for the single-launch forward.
    python3 tools/step_hash.py [k ..., default 8 40]
600 Zipf rows in 3 batches of 200 (the dense hot block on), 300 features, 1 to 12 entries per row; cuts at the shares (0.3, 0.6)
of the stored nonzeros.  Per route and k one line: the parameters after one step (of batch 2; the exchange modes: of position 0)
and after two more epochs.  The exchange modes run at world 2 as thread ranks on this GPU, rank 0 with 3 batches and rank 1
with one, which so runs out of rows."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparkfm_amd import DataSet, FMModel, HipBPR, HipSGD, Relation, RelationalData, _ffi, synth  # noqa: E402
from sparkfm_amd.distributed import HipDataParallelSGD, HipEngine, ThreadStagedComm, run_thread_ranks, torch_stream_handle  # noqa: E402

KS = [int(x) for x in sys.argv[1:]] or [8, 40]
ROWS, BATCH, N1 = 600, 200, 300
FRACTIONS = (0.3, 0.6)
ETA, DECAY, NO_DECAY = 0.05, dict(reg0=1e-3, regw=1e-3, regv=2e-3), dict(reg0=0.0, regw=0.0, regv=0.0)
L = _ffi.load()


def sha(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in arrays)).hexdigest()[:16]


def model(k, stream=None):
    rng = np.random.default_rng(1000 + k)
    fm = FMModel(N1 - 1, k, stream=stream)
    fm.w0, fm.w, fm.v = float(rng.normal(0, 0.1)), rng.normal(0, 0.1, N1), rng.normal(0, 0.1, (k, N1))
    return fm


def params(fm):
    fm._device_updated()
    return sha(fm.v, fm.w, np.float64(fm.w0))


def route(name, k, step, epoch, fm=None, before_close=lambda: None):
    """step(fm): one step; epoch(fm): one epoch; -> the line."""
    fm = fm or model(k)
    step(fm)
    first = params(fm)
    for _ in range(2):
        epoch(fm)
    print("%-24s k=%-3d one step %s | after 2 epochs %s" % (name, k, first, params(fm)))
    before_close()
    fm.close()


d = synth.make_zipf(2026, ROWS, N1, 1, 12, zipf_s=1.05)
ds = DataSet.from_arrays(d, batch_rows=BATCH).cache()
assert ds.layout()["hot_pages"] > 0
cnt = np.bincount(d["col"], minlength=N1)
above = np.cumsum(cnt[::-1])[::-1]
C1, C2 = sorted(int(np.argmax(above <= f * cnt.sum())) for f in FRACTIONS)
assert 0 < C1 < C2 < N1


def split_step(fm, b, ascending, regs):
    """fmhip_step_forward, fmhip_step_backward over the three intervals, fmhip_step_apply."""
    _ffi.check(L.fmhip_step_forward(fm.handle, ds.handle, b))
    cuts = [(0, C1), (C1, C2), (C2, N1)]
    for lo, hi in (cuts if ascending else cuts[::-1]):
        _ffi.check(L.fmhip_step_backward(fm.handle, ds.handle, b, lo, hi, 1 if lo == 0 else 0))
    _ffi.check(L.fmhip_step_apply(fm.handle, ETA, regs["reg0"], regs["regw"], regs["regv"]))


def two_pass_step(fm, b, regs):
    _ffi.check(L.fmhip_step_forward_pass(fm.handle, ds.handle, b, 0))
    _ffi.check(L.fmhip_step_forward_pass(fm.handle, ds.handle, b, 1))
    _ffi.check(L.fmhip_step_backward(fm.handle, ds.handle, b, 0, N1, 1))
    _ffi.check(L.fmhip_step_apply(fm.handle, ETA, regs["reg0"], regs["regw"], regs["regv"]))


def bound_step(eng, b, regs):
    eng.compute(b)
    eng.apply(ETA, regs["reg0"], regs["regw"], regs["regv"])


def exchange_route(exchange, k):
    cfg_rows = [ROWS, BATCH]

    def rank(r, group):
        dr = synth.make_zipf(2026, cfg_rows[r], N1, 1, 12, zipf_s=1.05, row_begin=int(sum(cfg_rows[:r])))
        dsr = DataSet.from_arrays(dr, batch_rows=BATCH).cache()
        fm = model(k)
        comm = ThreadStagedComm(fm, r, group)
        dp = HipDataParallelSGD(comm, eta=ETA, exchange=exchange, upper_fractions=FRACTIONS, **DECAY)
        dp.plan(fm, dsr)
        dp.step_at(fm, dsr, 0)
        first = params(fm)
        for _ in range(2):
            dp.learn(fm, dsr)
        out = first, params(fm)
        group.barrier()
        comm.close()
        dsr.unpersist()
        fm.close(discard=True)
        return out

    res = run_thread_ranks(2, rank)
    assert res[0] == res[1], (exchange, k, "the replicas differ")
    print("%-24s k=%-3d one step %s | after 2 epochs %s" % ("exchange " + exchange, k, res[0][0], res[0][1]))


# relational and BPR: the shapes of tools/finish_hash.py
rng = np.random.default_rng(5)


def rows_of(n, f0, f1, lo, hi):
    cnt_ = rng.integers(lo, hi + 1, n)
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(cnt_, out=ptr[1:])
    col = np.concatenate([rng.choice(f1 - f0, size=c, replace=False) + f0 for c in cnt_]).astype(np.int32)
    return ptr, col, rng.uniform(0.2, 1.0, ptr[-1])


yb = (rng.random(ROWS) < 0.4).astype(np.float64)
users = Relation(rows_of(40, 0, 100, 2, 9), rng.integers(0, 40, ROWS), name="users")
items = Relation(rows_of(25, 100, 200, 1, 6), rng.integers(0, 25, ROWS), name="items")
pp, pc, pv = rows_of(ROWS, 200, N1, 0, 5)
rd = RelationalData(yb, [users, items], plain=DataSet(pp, pc, pv, yb, batch_rows=BATCH, name="plain"), batch_rows=BATCH).cache()
key = np.sort(rng.choice(40 * 25, size=ROWS // 2, replace=False))
positives = [(key[key // 25 == u] % 25).astype(np.int32) for u in range(40)]

for k in KS:
    for name, regs in (("sgd decay", DECAY), ("sgd no decay", NO_DECAY)):
        sgd = HipSGD(eta=ETA, **regs)
        route(name, k, lambda fm: sgd.step(fm, ds, 2), lambda fm: sgd.learn(fm, ds))
    for name, asc in (("split descending", False), ("split ascending", True)):
        route(name, k, lambda fm: split_step(fm, 2, asc, DECAY), lambda fm: [split_step(fm, b, asc, DECAY) for b in range(3)])
    _ffi.check(L.fmhip_dataset_partition_rows(ds.handle, C2))
    route("two-pass forward", k, lambda fm: two_pass_step(fm, 2, DECAY), lambda fm: [two_pass_step(fm, b, DECAY) for b in range(3)])
    ada = HipSGD(eta=ETA, optimizer="adagrad", **DECAY)
    route("adagrad", k, lambda fm: ada.step(fm, ds, 2), lambda fm: ada.learn(fm, ds))
    fmb = model(k, stream=torch_stream_handle(0))
    eng = HipEngine(fmb, ds)
    route("bound gradient buffer", k, lambda fm: bound_step(eng, 2, DECAY), lambda fm: [bound_step(eng, b, DECAY) for b in range(3)], fm=fmb,
          before_close=eng.close)
    rel = HipSGD(eta=ETA, loss="logistic", **DECAY)
    route("relational + plain", k, lambda fm: rel.step(fm, rd, 2), lambda fm: rel.learn(fm, rd))
    bpr = HipBPR.run(users.block, items.block, positives, n_neg=1, batch_pairs=BATCH // 2, seed=3, eta=ETA, n_candidates=1, **DECAY)
    route("BPR uniform", k, lambda fm: bpr.step(fm, 2), bpr.learn)
    bpr.close()
    for exchange in ("dense", "touched", "sharded", "pipelined"):
        exchange_route(exchange, k)
