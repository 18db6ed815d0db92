"""fp64 twin of the BPR trainer's per-batch redraw (include/fmhip_redraw.h), built from the pieces of bpr_ref, bpr_adaptive_ref and
warp_ref, which it changes in nothing.

 - the candidates of a pair at epoch t do not depend on the model: bpr_adaptive_ref.candidates once per epoch (candidate 0 is
   bpr_ref's uniform draw);
 - per batch, in the order given: the score table under the twin's state AS IT STANDS, the choice for the batch's pairs alone
   (uniform: candidate 0; best of C: bpr_adaptive_ref.first_strict_max; WARP: warp_ref.first_violator / choose), written into the
   standing draw — the other pairs keep what they had — then the batch's step (bpr_ref.step, or warp_ref.step under WARP);
 - the per-epoch twin of the same samplers (`epochs` with redraw="epoch") is bpr_ref.epochs / bpr_adaptive_ref.epochs /
   warp_ref.epochs, called as they are: with one batch the two redraws are the same arithmetic in the same order."""
import numpy as np

import bpr_adaptive_ref as aref
import bpr_ref as bref
import relational_ref as rref
import warp_ref as wref

SAMPLERS = ("uniform", "best", "warp")


def sampler_of(C, warp):
    return "warp" if warp else "best" if C > 1 else "uniform"


class Draw:
    """The standing draw of every pair: negatives, and under WARP weights and trial counts."""

    def __init__(self, P, neg=None):
        n = len(P["ctx"]) * P["n_neg"]
        self.neg = bref.draw(P, 0)[0] if neg is None else np.array(neg, np.int32)      # (what fmhip_bpr_create leaves)
        self.weights = np.zeros(n, np.float32)
        self.trials = np.zeros(n, np.int32)


def choose(P, sampler, rows, ctx, pos, p0, p1, margin, w0, w, v):
    """The sampler's choice for the pairs [p0, p1) among their candidate rows `rows` [p1 - p0, C] under the parameters (w0, w, v)
    -> dict(neg; WARP: weights, trials; the sampler's counters that depend on the model)."""
    if sampler == "uniform":
        return dict(neg=rows[:, 0].astype(np.int32))
    T, _ = aref.score_table(w0, w, v, P["users"], P["items"])
    sc = T[ctx[p0:p1, None], rows]
    if sampler == "best":
        keep = aref.first_strict_max(sc)
        return dict(neg=rows[np.arange(p1 - p0), keep].astype(np.int32), replaced=int((keep != 0).sum()))
    n_first = wref.first_violator(sc, T[ctx[p0:p1], pos[p0:p1]], margin)
    neg, cw = wref.choose(rows, n_first, wref.weight_table(P["M"], rows.shape[1]))
    return dict(neg=neg, weights=cw, trials=n_first, violated=int((n_first > 0).sum()), sum_trials=int(n_first.sum()))


def batch_step(s, P, D, sampler, rows, r0, r1, margin, eta, reg0, regw, regv, rule):
    """Batch [r0, r1) (rows of the pair layout): its pairs redrawn under s into the standing draw D, then its step, in place
    -> the choice's dict."""
    ctx = np.repeat(P["ctx"], P["n_neg"]).astype(np.int64)
    pos = np.repeat(P["cand"], P["n_neg"]).astype(np.int64)
    p0, p1 = r0 // 2, r1 // 2
    got = choose(P, sampler, rows[p0:p1], ctx, pos, p0, p1, margin, s.w0, s.w, s.v)
    D.neg[p0:p1] = got["neg"]
    p = bref.layout(P, D.neg)
    if sampler == "warp":
        D.weights[p0:p1], D.trials[p0:p1] = got["weights"], got["trials"]
        wref.step(s, p, r0, r1, D.weights, margin, eta, reg0, regw, regv, rule, rref.parts_of(p))
    else:
        bref.step(s, p, r0, r1, eta, reg0, regw, regv, rule)
    return got


def epoch_candidates(P, t, C):
    """int32 [n_pairs, C]: every pair's candidate rows at epoch t (the per-epoch draw's)."""
    ctx = np.repeat(P["ctx"], P["n_neg"]).astype(np.int64)
    return aref.candidates(P["seed"], t, ctx, P["ptr"], P["rows"], P["M"], C)[0]


def epochs(s, P, n_epochs, batch_pairs, eta, reg0, regw, regv, rule, C, warp=False, margin=1.0, redraw="batch", t0=0, order=None):
    """Epochs t0 .. t0 + n_epochs - 1 of the sampler (uniform at C = 1, the best of C above, WARP with warp=True).  redraw="epoch":
    the existing twins.  redraw="batch": per batch in `order` (default ascending) the draw of its pairs under the state as it
    stands, then its step.  -> (s, Draw)."""
    sampler = sampler_of(C, warp)
    if redraw == "epoch":
        assert order is None
        if sampler == "warp":
            s, d = wref.epochs(s, P, n_epochs, batch_pairs, eta, reg0, regw, regv, rule, C, margin, t0)
            D = Draw(P, d["neg"])
            D.weights, D.trials = d["weights"], d["trials"]
            return s, D
        if sampler == "best":
            s, p = aref.epochs(s, P, n_epochs, batch_pairs, eta, reg0, regw, regv, rule, C, t0)
        else:
            s, p = bref.epochs(s, P, n_epochs, batch_pairs, eta, reg0, regw, regv, rule, t0)
        return s, Draw(P, p["maps"][1][1::2])
    assert redraw == "batch"
    D = Draw(P)
    bt = wref.batches(2 * len(D.neg), batch_pairs)
    for t in range(t0, t0 + n_epochs):
        rows = epoch_candidates(P, t, C)
        for b in (range(len(bt)) if order is None else order):
            batch_step(s, P, D, sampler, rows, bt[b][0], bt[b][1], margin, eta, reg0, regw, regv, rule)
    return s, D
