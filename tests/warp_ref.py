"""fp64 twin of WARP for the BPR trainer (include/fmhip_warp.h), on top of bpr_ref / bpr_adaptive_ref, which it changes in nothing.

 - the weight table: W[0] = 0, W[n] = float32(H(max(1, (M - 1) // n))), H(r) = sum_{j = 1 .. r} 1 / j in fp64 with j ascending;
 - the choice: thr = s+ - margin in the scores' own dtype (float32 arrays: one fp32 subtraction, the device's; float64: the twin's),
   candidate c violates iff s_c > thr (a tie and a NaN on either side do not), N = 1 + the lowest violating c, 0 for none; the kept
   row is the violator's, or candidate 0's when N = 0;
 - the draw: bpr_adaptive_ref's candidates and score table, the positive's score from the same table;
 - the step: bpr_ref's by-block gradient with the pair residual g_p = c_p * (-1 if d_p < margin else 0), e_2p = g_p, e_2p+1 = -g_p,
   |B| the row count; SGD or AdaGrad as train_ref's rule says (its loss is not read);
 - the epochs: at epoch t the draw against the state as it stands, then every batch."""
import numpy as np

import bpr_adaptive_ref as aref
import bpr_ref as bref
import relational_ref as rref
import train_ref as ref


def harmonic(r):
    h = 0.0
    for j in range(1, int(r) + 1):
        h += 1.0 / j
    return h


def weight_table(M, C):
    """float32 [C + 1]: W[0] = 0, W[n] the weight of a pair whose first violator is candidate n - 1."""
    return np.array([0.0] + [harmonic(max(1, (M - 1) // n)) for n in range(1, C + 1)]).astype(np.float32)


def first_violator(scores, s_pos, margin):
    """scores [n, C], s_pos [n] of one dtype -> N int32 [n]."""
    scores = np.asarray(scores)
    thr = np.asarray(s_pos, scores.dtype) - scores.dtype.type(margin)
    with np.errstate(invalid="ignore"):
        viol = scores > thr[:, None]          # (False for a NaN on either side)
    return np.where(viol.any(axis=1), viol.argmax(axis=1) + 1, 0).astype(np.int32)


def choose(rows, n_first, W):
    """-> (kept rows int32, weights float32) of the candidates `rows` [n, C] under the trial counts and the table."""
    rows = np.asarray(rows)
    keep = np.maximum(n_first, 1) - 1
    return rows[np.arange(len(rows)), keep].astype(np.int32), np.asarray(W, np.float32)[n_first]


def draw(P, t, C, margin, w0, w, v):
    """-> dict(neg, weights, trials [n_pairs], rows, scores, tol [n_pairs, C], pos_scores, pos_tol [n_pairs], gap [n_pairs, C] =
    s_c - (s+ - margin) in fp64, violated, sum_trials) of problem P at epoch t under the parameters (w0, w, v)."""
    ctx = np.repeat(P["ctx"], P["n_neg"]).astype(np.int64)
    pos = np.repeat(P["cand"], P["n_neg"]).astype(np.int64)
    rows, _, _ = aref.candidates(P["seed"], t, ctx, P["ptr"], P["rows"], P["M"], C)
    T, tol = aref.score_table(w0, w, v, P["users"], P["items"])
    sc, tl = T[ctx[:, None], rows], tol[ctx[:, None], rows]
    sp, tp = T[ctx, pos], tol[ctx, pos]
    n_first = first_violator(sc, sp, margin)
    neg, cw = choose(rows, n_first, weight_table(P["M"], C))
    return dict(neg=neg, weights=cw, trials=n_first, rows=rows, scores=sc, tol=tl, pos_scores=sp, pos_tol=tp, gap=sc - (sp - margin)[:, None],
                violated=int((n_first > 0).sum()), sum_trials=int(n_first.sum()))


def pair_g(d, cw, margin):
    """The weighted hinge's derivative in d: c * (-1 if d < margin else 0); a NaN d gives 0."""
    with np.errstate(invalid="ignore"):
        return np.asarray(cw, np.float64) * np.where(np.asarray(d) < margin, -1.0, 0.0)


def gradient(s, p, r0, r1, cw, margin, parts=None):
    """-> (G_w, G_V, e, d) of the rows [r0, r1) (whole pairs) of the layout p; cw: the weights of ALL pairs."""
    parts = rref.parts_of(p) if parts is None else parts
    yh, Q = rref.combine(s, parts, r0, r1)
    d = yh[0::2] - yh[1::2]
    g = pair_g(d, cw[r0 // 2:r1 // 2], margin)
    e = np.empty(r1 - r0)
    e[0::2], e[1::2] = g, -g
    gw, gv = np.zeros_like(s.w), np.zeros_like(s.v)
    for X, mp in parts:
        Pb, eb = np.zeros((X.shape[0], Q.shape[1])), np.zeros(X.shape[0])
        np.add.at(Pb, mp[r0:r1], e[:, None] * Q)
        np.add.at(eb, mp[r0:r1], e)
        gv += (X.T @ Pb).T - s.v * ((X * X).T @ eb)[None, :]
        gw += X.T @ eb
    return gw, gv, e, d


def step(s, p, r0, r1, cw, margin, eta, reg0, regw, regv, rule, parts=None):
    """One hinge step of the rows [r0, r1), in place (bpr_ref.step's update) -> (e, d) of the batch."""
    gw, gv, e, d = gradient(s, p, r0, r1, cw, margin, parts)
    b = float(r1 - r0)
    h0, hw, hv = reg0 * s.w0, gw / b + regw * s.w, gv / b + regv * s.v
    if rule.eps is None:
        s.w0, s.w, s.v = s.w0 - eta * h0, s.w - eta * hw, s.v - eta * hv
        return e, d
    t0, s.n0 = ref.adagrad_rule(np.float64(s.w0), np.float64(s.n0), h0, eta, rule.eps)
    s.w0 = float(t0)
    s.w, s.nw = ref.adagrad_rule(s.w, s.nw, hw, eta, rule.eps)
    s.v, s.nv = ref.adagrad_rule(s.v, s.nv, hv, eta, rule.eps)
    return e, d


def batches(n_rows, batch_pairs):
    br = 2 * batch_pairs if 0 < batch_pairs <= n_rows // 2 else n_rows
    return [(r0, min(n_rows, r0 + br)) for r0 in range(0, n_rows, br)]


def epochs(s, P, n_epochs, batch_pairs, eta, reg0, regw, regv, rule, C, margin=1.0, t0=0):
    """Epochs t0 .. t0 + n_epochs - 1: the WARP draw at t against the state as it stands, then every batch -> (s, the last draw)."""
    d = None
    for t in range(t0, t0 + n_epochs):
        d = draw(P, t, C, margin, s.w0, s.w, s.v)
        p = bref.layout(P, d["neg"])
        parts = rref.parts_of(p)
        for r0, r1 in batches(len(p["y"]), batch_pairs):
            step(s, p, r0, r1, d["weights"], margin, eta, reg0, regw, regv, rule, parts)
    return s, d
