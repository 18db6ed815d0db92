"""fp64 twin of the BPR trainer's adaptive negatives (include/fmhip_bpr_adaptive.h) and the tasks its tests share.

 - candidates: candidate c of pair p at epoch t is bpr_ref's sampler with the counter's group word offset — attempt a takes word
   a & 3 of the Philox block of counter (p, (c << 4) | (a >> 2), t, stream 6); the 64-attempt bound, the forced walk and "never a
   positive" as there.  Candidate 0 is bpr_ref.negative.
 - scores: s(u, i) = yhat(i) + <q_u, q_i> = topk_ref.pair_ref's S[u, i] minus the per-context constant yhat(u) - w0, with pair_ref's
   tolerance for the pair.
 - the choice: the first strict maximum in order of c (candidate 0 the incumbent; a NaN never replaces it).
 - the twin's epochs: bpr_ref.epochs with every epoch's negatives chosen against the state at the epoch's start.
 - `hard_task`: the planted preference task made harder — more items and a popularity-skewed planted item bias."""
import numpy as np

import bpr_ref as bref
import mcmc_ref
from topk_ref import pair_ref, row_stats

MAX_CANDIDATES = 64


def candidate(seed, p, c, t, M, lst):
    """One candidate, step by step -> (row, attempts, forced).  lst: the context's positives, ascending and distinct."""
    pos = set(int(x) for x in lst)
    row = 0
    for a in range(bref.MAX_ATTEMPTS):
        if a % 4 == 0:
            words = [int(x[0]) for x in mcmc_ref.philox(p, (c << 4) | (a // 4), t, bref.STREAM_NEGATIVE, *mcmc_ref.key_of(seed))]
        row = (words[a % 4] * M) >> 32
        if row not in pos:
            return row, a + 1, 0
    while row in pos:
        row = (row + 1) % M
    return row, bref.MAX_ATTEMPTS, 1


def candidates(seed, t, ctx, ptr, rows, M, C):
    """Every pair's C candidates at epoch t -> (int32 [n_pairs, C], attempts, forced), the sums over all candidates."""
    n = len(ctx)
    ctx = np.asarray(ctx)
    key = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr)) * M + np.asarray(rows[:ptr[-1]], np.int64)
    listed = lambda u, r: np.isin(u.astype(np.int64) * M + r, key)                                                           # noqa: E731
    out = np.zeros((n, C), np.int64)
    attempts = forced = 0
    for c in range(C):
        open_ = np.arange(n)
        for a in range(bref.MAX_ATTEMPTS):
            if not len(open_):
                break
            if a % 4 == 0:
                words = mcmc_ref.philox(open_, (c << 4) | (a // 4), t, bref.STREAM_NEGATIVE, *mcmc_ref.key_of(seed))
            r = ((words[a % 4] * np.uint64(M)) >> np.uint64(32)).astype(np.int64)
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


def score_table(w0, w, v, users, items):
    """-> (T [n_ctx, M], tol [n_ctx, M]): T[u, i] = yhat(i) + <q_u, q_i> in fp64 and the project's tolerance of the pair's score."""
    S, tol = pair_ref(w0, w, v, users, items)
    yc = row_stats(w0, w, v, users)[0]
    return S - (yc - w0)[:, None], tol


def first_strict_max(scores):
    """[n, C] -> the candidate index kept per row: candidate 0, replaced by every later candidate strictly greater than the incumbent."""
    scores = np.asarray(scores)
    keep = np.zeros(len(scores), np.int64)
    best = scores[:, 0].copy()
    for c in range(1, scores.shape[1]):
        better = scores[:, c] > best          # (False for a NaN on either side)
        keep[better], best[better] = c, scores[better, c]
    return keep


def draw(P, t, C, w0, w, v):
    """-> dict(neg [n_pairs], rows [n_pairs, C], scores [n_pairs, C], tol, keep, attempts, forced, replaced) of problem P at epoch t
    under the parameters (w0, w, v)."""
    ctx = np.repeat(P["ctx"], P["n_neg"]).astype(np.int64)
    rows, attempts, forced = candidates(P["seed"], t, ctx, P["ptr"], P["rows"], P["M"], C)
    T, tol = score_table(w0, w, v, P["users"], P["items"])
    sc, tl = T[ctx[:, None], rows], tol[ctx[:, None], rows]
    keep = first_strict_max(sc)
    neg = rows[np.arange(len(ctx)), keep]
    return dict(neg=neg.astype(np.int32), rows=rows, scores=sc, tol=tl, keep=keep, attempts=attempts, forced=forced, replaced=int((keep != 0).sum()))


def epochs(s, P, n_epochs, batch_pairs, eta, reg0, regw, regv, rule, C, t0=0):
    """bpr_ref.epochs with adaptive negatives: at epoch t the C candidates are scored against the state as it stands, then every batch."""
    p = None
    for t in range(t0, t0 + n_epochs):
        neg = draw(P, t, C, s.w0, s.w, s.v)["neg"] if C > 1 else bref.draw(P, t)[0]
        p = bref.layout(P, neg)
        n = len(p["y"])
        br = 2 * batch_pairs if 0 < batch_pairs <= n // 2 else n
        for r0 in range(0, n, br):
            bref.step(s, p, r0, min(n, r0 + br), eta, reg0, regw, regv, rule)
    return s, p


def margins(P, neg, w0, w, v):
    """fp64 yhat(u, i+) - yhat(u, i-) of every pair under the draw `neg` (the per-context terms cancel)."""
    T, _ = score_table(w0, w, v, P["users"], P["items"])
    ctx = np.repeat(P["ctx"], P["n_neg"]).astype(np.int64)
    pos = np.repeat(P["cand"], P["n_neg"]).astype(np.int64)
    return T[ctx, pos] - T[ctx, np.asarray(neg, np.int64)]


# ---- tasks ---------------------------------------------------------------------------------------------------------------------------

def hard_task(seed, n_users=60, n_items=400, per_user=20, k_true=4, held=0.25, amp=1.5):
    """bpr_ref.planted_task made harder: 400 items of which a user interacts with 20 (5 of them held out), and a planted item bias
    that follows a popularity law — the item of popularity rank r (a random permutation) gets amp * log(n_items / (1 + r)) /
    log(n_items) — so the head items fill every user's list and a uniform negative is almost always an easy tail item.
    -> dict(users, items, train, held_out, n1) as planted_task."""
    rng = np.random.default_rng(seed)
    pu, qi = rng.normal(0, 1.0, (n_users, k_true)), rng.normal(0, 1.0, (n_items, k_true))
    rank = rng.permutation(n_items)
    bi = amp * np.log(n_items / (1.0 + rank)) / np.log(n_items)
    score = pu @ qi.T + bi[None, :]
    onehot = lambda n, base: dict(row_ptr=np.arange(n + 1, dtype=np.int64), col=(base + np.arange(n)).astype(np.int32), val=np.ones(n))      # noqa: E731
    train, held_out = [], []
    for u in range(n_users):
        best = rng.permutation(np.argsort(-score[u])[:per_user])
        n_held = int(round(held * per_user))
        held_out.append(np.sort(best[:n_held]))
        train.append(np.sort(best[n_held:]))
    return dict(users=onehot(n_users, 0), items=onehot(n_items, n_users), train=train, held_out=held_out, n1=n_users + n_items)


def task_problem(T, seed, k, n_neg, scale=0.05):
    """The bpr_ref problem dict of a planted task: shuffled training order, w0 = w = 0, v ~ N(0, scale) from seed + 1000."""
    n_ctx, M = len(T["train"]), len(T["items"]["row_ptr"]) - 1
    ctx, cand, ptr, rows = bref.training_order(T["train"], M, seed, True)
    v0 = np.random.default_rng(seed + 1000).normal(0, scale, (k, T["n1"]))
    return dict(seed=seed, k=k, n1=T["n1"], M=M, n_ctx=n_ctx, n_neg=n_neg, shuffle=True, users=T["users"], items=T["items"], positives=T["train"],
                ctx=ctx, cand=cand, ptr=ptr, rows=rows, w0=0.0, w=np.zeros(T["n1"]), v=v0)


def twin_ndcg(T, P, s):
    """Held-out NDCG@10 of the state's scores over (users x items), the training items excluded."""
    tab, _ = score_table(s.w0, s.w, s.v, T["users"], T["items"])
    return bref.ndcg_at(tab, T["held_out"], T["train"])
