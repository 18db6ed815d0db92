#!/usr/bin/env python3
"""Prints hashes of what every route behind a q-mode forward computes (the finishes of fm_pairing.hip / fm_weights.hip /
fm_relational.hip, the BPR trainer's samplers) on fixed small data: run it with two builds of the library
(FMHIP_LIB=sparkfm_amd/lib/libfmhip_<name>.so, tools/build_variant.sh) to check that a change to those kernels or their launchers
left every bit where it was — tools/grad_hash.py does the same for the single-launch forward.
    python3 tools/finish_hash.py [k ..., default 8 32 48 64 100 128 200 256]
600 rows in 3 batches of 200 (the last workgroup of every finish has empty slots), 300 features.  Per case and k one line: the
flat routes hash batch 2's gradient (gv, gw) and print g0 and sse, the relational and BPR routes — which have no gradient call —
hash the parameters after one step of batch 2 and print that step's sum e and sse; then every route hashes the parameters after
two epochs.  The adaptive BPR case adds the statistics of one more draw under the trained model.  The lines of the scored samplers
(best of C at C = 9, WARP at C = 4 and 9, margin 0.1) hash the parameters after two epochs and, under that model at t = 2, what the
record call returns for all pairs (rows, scores, WARP: the positives' scores) and what a draw leaves (negatives, WARP: trials and
pair weights), with the draw's statistics."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sparkfm_amd import DataSet, FMModel, HipBPR, HipSGD, Relation, RelationalData, _ffi  # noqa: E402

KS = [int(x) for x in sys.argv[1:]] or [8, 32, 48, 64, 100, 128, 200, 256]
ROWS, BATCH, N1 = 600, 200, 300
ETA, REGS = 0.05, dict(reg0=1e-3, regw=1e-3, regv=2e-3)


def sha(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in arrays)).hexdigest()[:16]


def rows_of(rng, n, f0, f1, lo, hi):
    """n CSR rows of lo..hi distinct features of [f0, f1), values in [0.2, 1]."""
    cnt = rng.integers(lo, hi + 1, n)
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(cnt, out=ptr[1:])
    col = np.concatenate([rng.choice(f1 - f0, size=c, replace=False) + f0 for c in cnt]).astype(np.int32)
    return ptr, col, rng.uniform(0.2, 1.0, ptr[-1])


def model(k):
    rng = np.random.default_rng(1000 + k)
    fm = FMModel(N1 - 1, k)
    fm.w0, fm.w, fm.v = float(rng.normal(0, 0.1)), rng.normal(0, 0.1, N1), rng.normal(0, 0.1, (k, N1))
    return fm


def params(fm):
    return sha(fm.v, fm.w, np.float64(fm.w0))


def flat_case(name, k, ds, loss, pairs):
    fm = model(k)
    L = _ffi.load()
    _ffi.check(L.fmhip_model_set_loss(fm.handle, _ffi.loss_code(loss)))
    _ffi.check(L.fmhip_model_set_pairing(fm.handle, _ffi.pairing_code(pairs)))
    gv, gw, g0, st = fm.batchGradient(ds, 2)
    sgd = HipSGD(eta=ETA, loss=loss, pairs=pairs, **REGS)
    for _ in range(2):
        sgd.learn(fm, ds)
    print("%-22s k=%-3d gradient %s g0 %.17g sse %.17g | after 2 epochs %s" % (name, k, sha(gv, gw), g0, st["sse"], params(fm)))
    fm.close()


def stepped_case(name, k, step, learn, extra=lambda fm: ""):
    fm = model(k)
    st = step(fm)
    first = params(fm)
    for _ in range(2):
        learn(fm)
    print("%-22s k=%-3d one step %s sum_e %.17g sse %.17g | after 2 epochs %s%s" % (name, k, first, st["sum_e"], st["sse"], params(fm), extra(fm)))
    fm.close()


def sampler_case(name, k, cand, kw):
    """Two epochs, then under the trained model at t = 2: the record call's arrays for all pairs, and what a draw leaves."""
    bpr = HipBPR.run(users.block, items.block, positives, n_neg=1, batch_pairs=BATCH // 2, seed=3, eta=ETA, n_candidates=cand, **REGS, **kw)
    fm = model(k)
    for _ in range(2):
        bpr.learn(fm)
    record = bpr.warp_draws(fm, 2) if bpr.warp else bpr.candidate_draws(fm, 2)
    st = bpr.resample(2, fm)
    left = [bpr.negatives()] + ([bpr.trials(), bpr.pair_weights()] if bpr.warp else [])
    print("%-22s k=%-3d after 2 epochs %s | record at t=2 %s | draw at t=2 %s %s" % (
        name, k, params(fm), sha(*record), sha(*left), " ".join("%s=%d" % kv for kv in sorted(st.items()))))
    bpr.close()
    fm.close()


rng = np.random.default_rng(5)
rp, col, val = rows_of(rng, ROWS, 0, N1, 1, 12)
y = rng.normal(0, 1, ROWS)
yb = (rng.random(ROWS) < 0.4).astype(np.float64)
c = rng.choice([0.0, 0.25, 1.0, 3.5], size=ROWS, p=[0.2, 0.3, 0.25, 0.25])
flat = {
    "weighted rows": (DataSet(rp, col, val, yb, batch_rows=BATCH, weights=c).cache(), "logistic", False),
    "weighted rows squared": (DataSet(rp, col, val, y, batch_rows=BATCH, weights=c).cache(), "squared", False),
    "pairs": (DataSet(rp, col, val, yb, batch_rows=BATCH).cache(), "logistic", True),
    "weighted pairs": (DataSet(rp, col, val, y, batch_rows=BATCH, weights=np.repeat(c[0::2], 2)).cache(), "squared", True),
}
# relational: users over features [0, 100), items over [100, 200), the plain part over [200, 300)
users = Relation(rows_of(rng, 40, 0, 100, 2, 9), rng.integers(0, 40, ROWS), name="users")
items = Relation(rows_of(rng, 25, 100, 200, 1, 6), rng.integers(0, 25, ROWS), name="items")
pp, pc, pv = rows_of(rng, ROWS, 200, N1, 0, 5)
plain = DataSet(pp, pc, pv, yb, batch_rows=BATCH, name="plain")
relational = {"relational + plain": RelationalData(yb, [users, items], plain=plain, batch_rows=BATCH).cache(),
              "relational": RelationalData(yb, [users.remap(users.mapping), items.remap(items.mapping)], batch_rows=BATCH).cache()}
# BPR: 300 interactions of 40 contexts with 25 candidates, 100 pairs (200 rows) per batch
key = np.sort(rng.choice(40 * 25, size=ROWS // 2, replace=False))
positives = [(key[key // 25 == u] % 25).astype(np.int32) for u in range(40)]

for k in KS:
    for name, (ds, loss, pairs) in flat.items():
        flat_case(name, k, ds, loss, pairs)
    for name, rd in relational.items():
        sgd = HipSGD(eta=ETA, loss="logistic", **REGS)
        stepped_case(name, k, lambda fm: sgd.step(fm, rd, 2), lambda fm: sgd.learn(fm, rd))
    for name, cand in (("BPR uniform", 1), ("BPR adaptive C=4", 4)):
        bpr = HipBPR.run(users.block, items.block, positives, n_neg=1, batch_pairs=BATCH // 2, seed=3, eta=ETA, n_candidates=cand, **REGS)
        stepped_case(name, k, lambda fm: bpr.step(fm, 2), bpr.learn,
                     (lambda fm: " | draw at t=2 " + " ".join("%s=%d" % kv for kv in sorted(bpr.resample(2, fm).items()))) if cand > 1 else (lambda fm: ""))
        bpr.close()
    # the scored samplers' walk: C = 9 is a second pass of the 8-lane group at k = 8, ending inside a chunk
    for name, cand, kw in (("BPR best-of-C C=9", 9, {}), ("BPR WARP C=4", 4, dict(sampler="warp", margin=0.1)),
                           ("BPR WARP C=9", 9, dict(sampler="warp", margin=0.1))):
        sampler_case(name, k, cand, kw)
