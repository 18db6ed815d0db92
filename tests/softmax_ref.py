"""fp64 twin of the BPR trainer's sampled softmax (include/fmhip_softmax.h), on top of bpr_ref, bpr_proposal_ref, redraw_ref and
warp_ref, which it changes in nothing.

 - `logq`: lq[i] = float32(log(w_i / S)), S the weights summed index-ascending in fp64 — what fmhip_host.cpp's bpr_log_proposal
   builds; the twin then reads those float32 values, as the device does;
 - `rule`: interaction j of n adjacent pairs with margins d_q: a_q = -d_q - (lq[i-_q] - lq[i+]), mx = max(0, a), Z = exp(-mx) +
   sum exp(a_q - mx), pi_q = exp(a_q - mx) / Z, g_q = -pi_q, loss_j = mx + log Z; an interaction with a non-finite d_q has every
   g_q = 0, loss 0, and is not on top;
 - the step: bpr_ref's by-block gradient with e_2p = g_p, e_2p+1 = -g_p, |B| the row count, the rows of a pair with g = 0 adding
   exact zeros (whatever their q holds); SGD or AdaGrad as train_ref's rule says (its loss is not read);
 - the epochs: at epoch t the C candidates of every pair — uniform (bpr_adaptive_ref.candidates) or from the alias table
   (bpr_proposal_ref.candidates) — the sampler's choice (redraw_ref.choose: candidate 0, or the best of C) against the state at
   the epoch's start (redraw="epoch") or at the batch's own step (redraw="batch"), then the batch's step."""
import numpy as np

import bpr_adaptive_ref as aref
import bpr_proposal_ref as pref
import bpr_ref as bref
import redraw_ref as dref
import relational_ref as rref
import train_ref as ref
import warp_ref as wref


def logq(weights):
    """float32 [M]: log(w_i / S), S summed index-ascending."""
    w = [float(x) for x in weights]
    total = 0.0
    for x in w:
        total += x
    # (a quotient that underflows to 0 takes the difference of the logs, as the library does: every entry is finite)
    return np.array([np.log(x / total) if x / total > 0 else np.log(x) - np.log(total) for x in w], np.float64).astype(np.float32)


def rule(d, n, corr=None):
    """d [pairs] (whole interactions of n), corr [pairs] = lq[negative] - lq[positive] or None
    -> (g [pairs], loss [interactions], top [interactions] bool)."""
    d = np.asarray(d, np.float64).reshape(-1, n)
    a = -d if corr is None else -d - np.asarray(corr, np.float64).reshape(-1, n)
    ok = np.isfinite(d).all(axis=1)
    a_ok = np.where(ok[:, None], a, 0.0)
    mx = np.maximum(0.0, a_ok.max(axis=1))
    ex = np.exp(a_ok - mx[:, None])
    Z = np.exp(-mx) + ex.sum(axis=1)
    pi = np.where(ok[:, None], ex / Z[:, None], 0.0)
    loss = np.where(ok, mx + np.log(Z), 0.0)
    top = ok & (a_ok < 0).all(axis=1)
    return -pi.reshape(-1), loss, top


def corrections(p, r0, r1, lq):
    """lq[negative] - lq[positive] of the pairs of rows [r0, r1) of the layout p (the float32 table's values in fp64), or None."""
    if lq is None:
        return None
    mi = np.asarray(p["maps"][1][r0:r1], np.int64)
    lq = np.asarray(lq, np.float32)
    return (lq[mi[1::2]] - lq[mi[0::2]]).astype(np.float64)      # (one fp32 subtraction, as the device forms it)


def block_caches(s, X):
    """relational_ref.block_caches, with a non-finite row of v reaching only the block rows that hold its feature (a dense product
    would spread 0 * NaN over every row): those rows' q and yhat are NaN, the others are computed without it."""
    fin = np.isfinite(s.v).all(axis=0)
    if fin.all():
        return rref.block_caches(s, X)
    t = s.copy()
    t.v = np.where(fin[None, :], s.v, 0.0)
    q, yb = rref.block_caches(t, X)
    hit = (X[:, ~fin] != 0).any(axis=1)
    q[hit], yb[hit] = np.nan, np.nan
    return q, yb


def combine(s, parts, r0, r1):
    """relational_ref.combine over those caches -> (yhat [r1 - r0], Q [r1 - r0, k])."""
    Q = np.zeros((r1 - r0, s.v.shape[0]))
    yh = np.full(r1 - r0, s.w0)
    for X, mp in parts:
        q, yb = block_caches(s, X)
        j = mp[r0:r1]
        yh += (yb[j] - s.w0) + (q[j] * Q).sum(1)
        Q += q[j]
    return yh, Q


def gradient(s, p, r0, r1, n, lq=None, parts=None):
    """-> (G_w, G_V, e, loss [interactions], top) of the rows [r0, r1) (whole interactions) of the layout p."""
    parts = rref.parts_of(p) if parts is None else parts
    with np.errstate(invalid="ignore"):
        yh, Q = combine(s, parts, r0, r1)
        g, loss, top = rule(yh[0::2] - yh[1::2], n, corrections(p, r0, r1, lq))
    e = np.empty(r1 - r0)
    e[0::2], e[1::2] = g, -g
    with np.errstate(invalid="ignore"):
        eQ = np.where(e[:, None] != 0.0, e[:, None] * Q, 0.0)
    gw, gv = np.zeros_like(s.w), np.zeros_like(s.v)
    for X, mp in parts:
        Pb, eb = np.zeros((X.shape[0], Q.shape[1])), np.zeros(X.shape[0])
        np.add.at(Pb, mp[r0:r1], eQ)
        np.add.at(eb, mp[r0:r1], e)
        with np.errstate(invalid="ignore"):
            gv += (X.T @ Pb).T - s.v * ((X * X).T @ eb)[None, :]
        gw += X.T @ eb
    return gw, gv, e, loss, top


def step(s, p, r0, r1, n, eta, reg0, regw, regv, rule_, lq=None, parts=None):
    """One softmax step of the rows [r0, r1), in place (bpr_ref.step's update) -> (e, loss, top) of the batch."""
    gw, gv, e, loss, top = gradient(s, p, r0, r1, n, lq, parts)
    b = float(r1 - r0)
    h0, hw, hv = reg0 * s.w0, gw / b + regw * s.w, gv / b + regv * s.v
    if rule_.eps is None:
        s.w0, s.w, s.v = s.w0 - eta * h0, s.w - eta * hw, s.v - eta * hv
        return e, loss, top
    t0, s.n0 = ref.adagrad_rule(np.float64(s.w0), np.float64(s.n0), h0, eta, rule_.eps)
    s.w0 = float(t0)
    s.w, s.nw = ref.adagrad_rule(s.w, s.nw, hw, eta, rule_.eps)
    s.v, s.nv = ref.adagrad_rule(s.v, s.nv, hv, eta, rule_.eps)
    return e, loss, top


def score(s, p, n, lq=None):
    """-> (mean loss over the interactions, share on top) of the layout's pairs at the state's parameters."""
    yh = combine(s, rref.parts_of(p), 0, len(p["y"]))[0]
    _, loss, top = rule(yh[0::2] - yh[1::2], n, corrections(p, 0, len(yh), lq))
    return float(loss.mean()), float(top.mean())


def epochs(s, P, n_epochs, batch_pairs, eta, reg0, regw, regv, rule_, lq=None, table=None, C=1, redraw="epoch", t0=0):
    """Epochs t0 .. t0 + n_epochs - 1 -> (s, dict(neg, pi [n_pairs] as each batch's last step left it, sse of the last epoch))."""
    ctx = np.repeat(P["ctx"], P["n_neg"]).astype(np.int64)
    pos = np.repeat(P["cand"], P["n_neg"]).astype(np.int64)
    n = P["n_neg"]
    sampler = dref.sampler_of(C, False)
    neg = bref.draw(P, 0)[0].copy()                  # (what fmhip_bpr_create leaves)
    pi = np.zeros(len(ctx))
    sse = 0.0
    bt = wref.batches(2 * len(ctx), batch_pairs)
    assert all((r1 - r0) % (2 * n) == 0 for r0, r1 in bt)
    for t in range(t0, t0 + n_epochs):
        if table is None:
            rows = aref.candidates(P["seed"], t, ctx, P["ptr"], P["rows"], P["M"], C)[0]
        else:
            rows = pref.candidates(P["seed"], t, ctx, P["ptr"], P["rows"], P["M"], C, table)[0]
        if redraw == "epoch":
            neg = dref.choose(P, sampler, rows, ctx, pos, 0, len(ctx), 0.0, s.w0, s.w, s.v)["neg"].copy()
        sse = 0.0
        for r0, r1 in bt:
            p0, p1 = r0 // 2, r1 // 2
            if redraw == "batch":
                neg[p0:p1] = dref.choose(P, sampler, rows[p0:p1], ctx, pos, p0, p1, 0.0, s.w0, s.w, s.v)["neg"]
            p = bref.layout(P, neg)
            e, _, _ = step(s, p, r0, r1, n, eta, reg0, regw, regv, rule_, lq)
            pi[p0:p1] = -e[0::2]
            sse += float((e * e).sum())
    return s, dict(neg=neg, pi=pi, sse=sse)
