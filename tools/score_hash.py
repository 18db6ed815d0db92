#!/usr/bin/env python3
"""Prints hashes of what every READ call of the C ABI returns on fixed synthetic data — the scoring calls (predictions, residuals,
q, RMSE / log-loss / pairwise log-loss, AUC, top-K, pair scores, ranks), the parameter and optimizer-state reads, the batch gradient —
one line per case: a SHA-256 prefix of each result array, %.17g of each scalar.  Run it with two builds of the library
(FMHIP_LIB=sparkfm_amd/lib/libfmhip_<name>.so, tools/build_variant.sh): a change to the host side of those calls that moves no
arithmetic leaves every line as it was.  The sibling of tools/grad_hash.py, which covers training.
    python3 tools/score_hash.py
Cases: dense hot block on / off  x  k = 8 (packed rows, Kp = 32), 32 (unpacked, Kp = 32), 65 (packed, Kp = 128: 16-lane slots)  x
parameters as injected / after one SGD epoch with weight decay; k = 8 once more after an AdaGrad epoch, for the optimizer state.
1,000 rows x 300 features in batches of 384, 384 and 232 rows.  The model is 1,001 features wide, so that a batch touches less than
half of it and the SGD epoch's decay stays in the tables' scales (lazy decay): the reads then see sv, sw != 1."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import sparkfm_amd as fmhip  # noqa: E402
from sparkfm_amd import _ffi, synth  # noqa: E402

ROWS, FEATURES, BATCH, N_ATTR, CAND_ROWS, TOP = 1000, 300, 384, 1000, 500, 5


def sha(*arrays):
    return hashlib.sha256(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()[:12]


def stats_str(st):
    return "sse %.17g sum_e %.17g rows %d nnz %d nonfinite %d steps %d" % (st.sse, st.sum_e, st.rows, st.nnz, st.nonfinite, st.steps)


def auc_str(r):
    return "u2 %d pairs %d pos %d neg %d groups %d scored %d auc %.17g gauc %.17g" % (
        r["u2"], r["pairs"], r["positives"], r["negatives"], r["groups"], r["groups_scored"], r["auc"], r["gauc"])


def reads(fm, ds, cand, d, adagrad):
    """every read call on (fm, ds) -> the fields of one output line"""
    L, hm, hd = _ffi.load(), fm.handle, ds.handle
    n1, k = fm.num_attribute + 1, fm.num_factor
    rng = np.random.default_rng(5)
    out = []
    yhat = fm.predict(ds)
    out.append("predict %s" % sha(yhat))
    yrows = np.empty(ROWS)
    _ffi.check(L.fmhip_predict_rows(hm, ROWS, _ffi.ptr(d["row_ptr"]), _ffi.ptr(d["col"]), _ffi.ptr(d["val"].astype(np.float64)), _ffi.ptr(yrows)))
    out.append("predict_rows %s" % sha(yrows))
    out.append("residual %s" % sha(fm.residual(ds)))
    out.append("term_q %s" % sha(fm.termQ(ds)))
    for name in ("rmse", "logloss"):
        r, st = C.c_double(), _ffi.Stats()
        _ffi.check(getattr(L, "fmhip_" + name)(hm, hd, C.byref(r), C.byref(st)))
        out.append("%s %.17g %s" % (name, r.value, stats_str(st)))
    r, c, st = C.c_double(), C.c_double(), _ffi.Stats()
    _ffi.check(L.fmhip_pair_logloss(hm, hd, C.byref(r), C.byref(c), C.byref(st)))
    out.append("pair_logloss %.17g concordance %.17g %s" % (r.value, c.value, stats_str(st)))
    groups = rng.integers(0, 37, ROWS).astype(np.int32)
    for tag, g in (("auc", None), ("auc37", groups)):
        res = fm.aucDetails(ds, g, stats=True)
        st = _ffi.Stats(**res.pop("stats"))
        out.append("%s %s %s" % (tag, auc_str(res), stats_str(st)))
    res = _ffi.AucResult()
    _ffi.check(L.fmhip_auc_scores(0, ROWS, _ffi.ptr(yhat.astype(np.float32)), _ffi.ptr(ds.y.astype(np.float32)), _ffi.ptr(groups), C.byref(res)))
    out.append("auc_scores %s" % auc_str(res.as_dict()))
    exclude = [rng.choice(CAND_ROWS, rng.integers(0, 4), replace=False) for _ in range(ROWS)]
    idx, score = fm.recommend(ds, cand, TOP, exclude=exclude)
    out.append("topk %s %s" % (sha(idx), sha(score)))
    out.append("pair_scores %s" % sha(fm.pairScores(ds, cand, 300, 500)))
    # two relevant rows per context, none of them among the context's exclusions
    rel_rng = np.random.default_rng(6)       # (its own stream: the draws below stay what they were)
    relevant = [np.setdiff1d(rel_rng.choice(CAND_ROWS, 6, replace=False), e)[:2] for e in exclude]
    for tag, ex in (("rank_of", None), ("rank_of_excl", exclude)):
        ranks, scores = fm.rankOf(ds, cand, relevant, exclude=ex, scores=True)
        out.append("%s %s %s" % (tag, sha(*ranks), sha(*scores)))
    w0, w, v = C.c_double(), np.empty(n1), np.empty(n1 * k)
    _ffi.check(L.fmhip_model_get_params(hm, C.byref(w0), _ffi.ptr(w), _ffi.ptr(v)))
    out.append("get_params %.17g %s %s" % (w0.value, sha(w), sha(v)))
    f0, fw, fv = C.c_float(), np.empty(n1, np.float32), np.empty(n1 * k, np.float32)
    _ffi.check(L.fmhip_model_get_params_f32(hm, C.byref(f0), _ffi.ptr(fw), _ffi.ptr(fv)))
    out.append("get_params_f32 %.17g %s %s" % (f0.value, sha(fw), sha(fv)))
    ids = np.concatenate([[0, fm.num_attribute], rng.choice(np.arange(1, fm.num_attribute), 15, replace=False)]).astype(np.int32)
    out.append("get_rows %s %s" % tuple(sha(a) for a in fm.rows(ids)))
    gv, gw, g0, st = fm.batchGradient(ds, 1)
    out.append("batch_grad %s %s g0 %.17g %s" % (sha(gv), sha(gw), g0, stats_str(_ffi.Stats(**st))))
    if adagrad:
        def state():
            n0, nw, nv = C.c_double(), np.empty(n1), np.empty(n1 * k)
            _ffi.check(L.fmhip_model_get_optimizer_state(hm, C.byref(n0), _ffi.ptr(nw), _ffi.ptr(nv)))
            return n0.value, nw, nv
        n0, nw, nv = state()
        _ffi.check(L.fmhip_model_set_optimizer_state(hm, n0, _ffi.ptr(nw), _ffi.ptr(nv)))
        back = state()
        out.append("optimizer_state %.17g %s %s round trip %s" % (n0, sha(nw), sha(nv), "same" if sha(*back[1:]) == sha(nw, nv) and back[0] == n0 else "DIFFERS"))
    return out


def main():
    d = synth.make_zipf(7, ROWS, FEATURES, 4, 12, zipf_s=1.05)
    dc = synth.make_zipf(8, CAND_ROWS, FEATURES, 4, 12, zipf_s=1.05)
    cand = fmhip.DataSet.from_arrays(dc, scoring=True).cache()
    for hot in (True, False):
        ds = fmhip.DataSet.from_arrays(d, batch_rows=BATCH, hot_block=hot).cache()
        for k, state in [(k, s) for k in (8, 32, 65) for s in ("injected", "sgd")] + [(8, "adagrad")]:
            fm = fmhip.FMModel(N_ATTR, k)
            rng = np.random.Generator(np.random.PCG64(11 + k))
            fm.w0, fm.w, fm.v = 0.1, rng.normal(0.0, 0.05, N_ATTR + 1), rng.normal(0.0, 0.05, (k, N_ATTR + 1))
            if state == "sgd":
                fmhip.HipSGD(eta=0.05, regw=1e-3, regv=1e-3).learn(fm, ds)
            elif state == "adagrad":
                fmhip.HipSGD(eta=0.05, optimizer="adagrad").learn(fm, ds)
            print("hot=%d k=%d %s: %s" % (hot, k, state, " | ".join(reads(fm, ds, cand, d, state == "adagrad"))), flush=True)
            fm.close(discard=True)
        ds.unpersist()
    cand.unpersist()


if __name__ == "__main__":
    main()
