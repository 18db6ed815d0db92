"""fp64 twin of the BPR trainer's weighted proposal (include/fmhip_proposal.h), built on bpr_ref's Philox, which it changes in nothing.

 - `alias_table`: Vose's method in the order the header states — S = the weights summed index-ascending, q_i = w_i / S * M, the
   small (q < 1) and large lists index-ascending and used as stacks, bucket l = {floor(q_l * 2^32) clamped to 2^32 - 1, g},
   q_g = (q_g + q_l) - 1; what is left keeps its own row: {2^32 - 1, itself}.  Python floats are the C doubles, operation for
   operation, so the table is the library's entry for entry;
 - `proposal_row`: attempt a = 0 .. 31 of candidate c of pair p at epoch t takes words x0 = x[2 (a & 1)], x1 = x[2 (a & 1) + 1] of
   the Philox block of counter (p, (c << 4) | (a >> 1), t, stream 6): j = (x0 * M) >> 32, row = j if x1 < thresh[j] else alias[j],
   accepted unless it is a positive of the context; after 32 rejections the row steps up (mod M) until it is no positive: forced;
 - `candidates` / `sample`: the same rule for all pairs at once, as bpr_adaptive_ref.candidates / bpr_ref.sample;
 - `implied`: the probability the table gives every row, in exact integer arithmetic;
 - `popularity`: the weights of negatives="popularity"."""
from fractions import Fraction

import numpy as np

import bpr_ref as bref
import mcmc_ref
import redraw_ref as dref
import relational_ref as rref
import warp_ref as wref

MAX_ATTEMPTS = 32
TWO32 = 1 << 32


def alias_table(weights):
    """-> (thresh uint32 [M], alias int32 [M])."""
    w = [float(x) for x in weights]
    M = len(w)
    assert all(np.isfinite(x) and x > 0 for x in w)
    total = 0.0
    for x in w:
        total += x
    q = [x / total * float(M) for x in w]
    small = [i for i in range(M) if q[i] < 1.0]
    large = [i for i in range(M) if not q[i] < 1.0]
    thresh, alias = [TWO32 - 1] * M, list(range(M))
    while small and large:
        l, g = small.pop(), large.pop()
        thresh[l], alias[l] = min(int(np.floor(q[l] * 4294967296.0)), TWO32 - 1), g
        q[g] = (q[g] + q[l]) - 1.0
        (small if q[g] < 1.0 else large).append(g)
    return np.array(thresh, np.uint32), np.array(alias, np.int32)


def implied(thresh, alias):
    """The probability of every row under the table, as exact Fractions: a bucket keeps thresh / 2^32 of its 1 / M for its own row
    and gives the rest to its alias; a bucket whose alias is itself keeps everything."""
    M = len(thresh)
    mass = [0] * M
    for j in range(M):
        if int(alias[j]) == j:
            mass[j] += TWO32
        else:
            mass[j] += int(thresh[j])
            mass[int(alias[j])] += TWO32 - int(thresh[j])
    return [Fraction(m, M * TWO32) for m in mass]


def popularity(P, power=0.75, smooth=1.0):
    """(n_i + smooth) ** power, n_i the contexts whose positives list row i (a list's rows are distinct)."""
    counts = np.bincount(np.asarray(P["rows"][:P["ptr"][-1]], np.int64), minlength=P["M"]).astype(np.float64)
    return (counts + float(smooth)) ** float(power)


def proposal_row(seed, p, c, t, M, table, lst):
    """One candidate, step by step -> (row, attempts, forced).  lst: the context's positives, ascending and distinct."""
    thresh, alias = table
    pos = set(int(x) for x in lst)
    row = 0
    for a in range(MAX_ATTEMPTS):
        if a % 2 == 0:
            words = [int(x[0]) for x in mcmc_ref.philox(p, (c << 4) | (a // 2), t, bref.STREAM_NEGATIVE, *mcmc_ref.key_of(seed))]
        x0, x1 = words[2 * (a % 2)], words[2 * (a % 2) + 1]
        j = (x0 * M) >> 32
        row = j if x1 < int(thresh[j]) else int(alias[j])
        if row not in pos:
            return row, a + 1, 0
    while row in pos:
        row = (row + 1) % M
    return row, MAX_ATTEMPTS, 1


def candidates(seed, t, ctx, ptr, rows, M, C, table):
    """Every pair's C candidates at epoch t -> (int32 [n_pairs, C], attempts, forced), the sums over all candidates."""
    thresh, alias = np.asarray(table[0], np.uint64), np.asarray(table[1], np.int64)
    n = len(ctx)
    ctx = np.asarray(ctx)
    key = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr)) * M + np.asarray(rows[:ptr[-1]], np.int64)
    listed = lambda u, r: np.isin(u.astype(np.int64) * M + r, key)                                                           # noqa: E731
    out = np.zeros((n, C), np.int64)
    attempts = forced = 0
    for c in range(C):
        open_ = np.arange(n)
        for a in range(MAX_ATTEMPTS):
            if not len(open_):
                break
            if a % 2 == 0:
                words = mcmc_ref.philox(open_, (c << 4) | (a // 2), t, bref.STREAM_NEGATIVE, *mcmc_ref.key_of(seed))
            x0, x1 = words[2 * (a % 2)], words[2 * (a % 2) + 1]
            j = ((x0 * np.uint64(M)) >> np.uint64(32)).astype(np.int64)
            r = np.where(x1 < thresh[j], j, alias[j])
            out[open_, c] = r
            attempts += len(open_)
            rej = listed(ctx[open_], r)
            open_, words = open_[rej], tuple(w[rej] for w in words)
        for p in open_:
            lst = set(int(x) for x in rows[ptr[ctx[p]]:ptr[ctx[p] + 1]])
            r = int(out[p, c])
            while r in lst:
                r = (r + 1) % M
            out[p, c] = r
        forced += len(open_)
    return out.astype(np.int32), attempts, forced


def sample(seed, t, ctx, ptr, rows, M, table):
    """Every pair's negative at epoch t -> (int32 [n_pairs], attempts, forced), as bpr_ref.sample: candidate 0."""
    out, attempts, forced = candidates(seed, t, ctx, ptr, rows, M, 1, table)
    return out[:, 0].copy(), attempts, forced


def draw(P, t, table):
    """-> (negatives, attempts, forced) of the problem at epoch t under the table, as bpr_ref.draw."""
    return sample(P["seed"], t, np.repeat(P["ctx"], P["n_neg"]), P["ptr"], P["rows"], P["M"], table)


def epochs(s, P, n_epochs, batch_pairs, eta, reg0, regw, regv, rule, table, C=1, warp=False, margin=1.0, t0=0):
    """The per-epoch twins (bpr_ref.epochs at C = 1, bpr_adaptive_ref.epochs above, warp_ref.epochs with warp=True) with every
    candidate row drawn from the table: at epoch t the C candidates, the sampler's choice among them against the state as it stands
    (redraw_ref.choose), then every batch -> (s, dict(neg; WARP: weights, trials))."""
    ctx = np.repeat(P["ctx"], P["n_neg"]).astype(np.int64)
    pos = np.repeat(P["cand"], P["n_neg"]).astype(np.int64)
    got = None
    for t in range(t0, t0 + n_epochs):
        rows = candidates(P["seed"], t, ctx, P["ptr"], P["rows"], P["M"], C, table)[0]
        got = dref.choose(P, dref.sampler_of(C, warp), rows, ctx, pos, 0, len(ctx), margin, s.w0, s.w, s.v)
        p = bref.layout(P, got["neg"])
        parts = rref.parts_of(p)
        for r0, r1 in wref.batches(len(p["y"]), batch_pairs):
            if warp:
                wref.step(s, p, r0, r1, got["weights"], margin, eta, reg0, regw, regv, rule, parts)
            else:
                bref.step(s, p, r0, r1, eta, reg0, regw, regv, rule)
    return s, got
