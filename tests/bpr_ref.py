"""fp64 twin of the BPR trainer (include/fmhip_bpr.h) and the problems its tests share.

 - the sampler: attempt a = 0 .. 63 of pair p at epoch t takes word a & 3 of the Philox block of counter (p, a >> 2, t, stream 6)
   (mcmc_ref.philox, written from the paper), c = (word * M) >> 32, accepted unless c is a positive of the pair's context; after 64
   rejections c steps up (mod M) from the last c until it is no positive, and the pair counts as forced;
 - `append_batch`: RelationInverse::append_batch restated in Python — the inverse map of one batch and its work list at the cut;
 - the step: relational_ref's by-block-caches step on the pair layout (rows 2p / 2p+1 = context ++ positive / negative, labels
   1 / 0) with the pair residual e_2p = g_p, e_2p+1 = -g_p of train_ref.  test_host_bpr.py pins it to train_ref.step on the flat
   expansion to 1e-12."""
import numpy as np

import mcmc_ref
import relational_ref as rref
import train_ref as ref

STREAM_NEGATIVE = 6
MAX_ATTEMPTS = 64
CUT = 256


# ---- the sampler ----------------------------------------------------------------------------------------------------------

def negative(seed, p, t, M, lst):
    """One pair, step by step -> (row, attempts, forced).  lst: the context's positives, ascending and distinct."""
    pos = set(int(x) for x in lst)
    c = 0
    for a in range(MAX_ATTEMPTS):
        if a % 4 == 0:
            words = [int(x[0]) for x in mcmc_ref.philox(p, a // 4, t, STREAM_NEGATIVE, *mcmc_ref.key_of(seed))]
        c = (words[a % 4] * M) >> 32
        if c not in pos:
            return c, a + 1, 0
    while c in pos:
        c = (c + 1) % M
    return c, MAX_ATTEMPTS, 1


def sample(seed, t, ctx, ptr, rows, M):
    """Every pair's negative at epoch t -> (int32 [n_pairs], attempts, forced).  ctx: the pairs' contexts; ptr / rows: the
    contexts' positives.  The same rule as `negative`, all pairs at once."""
    n = len(ctx)
    key = np.repeat(np.arange(len(ptr) - 1, dtype=np.int64), np.diff(ptr)) * M + np.asarray(rows[:ptr[-1]], np.int64)      # ascending
    listed = lambda u, c: np.isin(u.astype(np.int64) * M + c, key)                                                           # noqa: E731
    out = np.zeros(n, np.int64)
    open_ = np.arange(n)
    attempts = 0
    for a in range(MAX_ATTEMPTS):
        if not len(open_):
            break
        if a % 4 == 0:
            words = mcmc_ref.philox(open_, a // 4, t, STREAM_NEGATIVE, *mcmc_ref.key_of(seed))
        c = ((words[a % 4] * np.uint64(M)) >> np.uint64(32)).astype(np.int64)
        out[open_] = c
        attempts += len(open_)
        rej = listed(np.asarray(ctx)[open_], c)
        open_, words = open_[rej], tuple(w[rej] for w in words)
    for p in open_:
        lst = set(int(x) for x in rows[ptr[ctx[p]]:ptr[ctx[p] + 1]])
        c = int(out[p])
        while c in lst:
            c = (c + 1) % M
        out[p] = c
    return out.astype(np.int32), attempts, len(open_)


# ---- the inverse map ---------------------------------------------------------------------------------------------------------

def append_batch(mapping, cut=CUT):
    """-> dict of trow, tptr, tj, wt, wbeg, wdst, lt, lfirst, lcount (int32) and counts = [n_touched, n_work, n_long, n_part]."""
    mapping = np.asarray(mapping, np.int64)
    tj = np.unique(mapping)
    trow = np.argsort(mapping, kind="stable")
    lens = np.bincount(mapping)[tj]
    tptr = np.concatenate([[0], np.cumsum(lens)])
    wt, wbeg, wdst, lt, lfirst, lcount = [], [], [], [], [], []
    n_part = 0
    for t, (j, ln, at) in enumerate(zip(tj, lens, tptr[:-1])):
        if ln <= cut:
            wt.append(t), wbeg.append(at), wdst.append(j)
        else:
            chunks = -(-ln // cut)
            lt.append(t), lfirst.append(n_part), lcount.append(chunks)
            for o in range(chunks):
                wt.append(t), wbeg.append(at + o * cut), wdst.append(-1 - n_part)
                n_part += 1
    i32 = lambda x: np.asarray(x, np.int32)      # noqa: E731
    return dict(trow=i32(trow), tptr=i32(tptr), tj=i32(tj), wt=i32(wt), wbeg=i32(wbeg), wdst=i32(wdst), lt=i32(lt), lfirst=i32(lfirst),
                lcount=i32(lcount), counts=i32([len(tj), len(wt), len(lt), n_part]))


# ---- the pair layout and its step -----------------------------------------------------------------------------------------------

def training_order(positives, M, seed, shuffle):
    """-> (ctx, cand, ptr, rows): the interactions in training order (context-ascending, rows ascending and distinct inside a context;
    shuffle: a PCG64([seed]) permutation of that) and the contexts' positives."""
    lists = [np.unique(np.asarray(x, np.int64)) for x in positives]
    ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    rows = np.concatenate(lists).astype(np.int32) if ptr[-1] else np.zeros(0, np.int32)
    ctx = np.repeat(np.arange(len(lists)), np.diff(ptr)).astype(np.int32)
    cand = rows.copy()
    if shuffle:
        perm = np.random.Generator(np.random.PCG64([seed])).permutation(len(ctx))
        ctx, cand = ctx[perm], cand[perm]
    return ctx, cand, ptr, rows


def layout(P, neg):
    """The relational problem (relational_ref's dict) the trainer stands for under the draw `neg`."""
    n_pairs = len(neg)
    ctx, pos = np.repeat(P["ctx"], P["n_neg"]), np.repeat(P["cand"], P["n_neg"])
    mi = np.empty(2 * n_pairs, np.int32)
    mi[0::2], mi[1::2] = pos, neg
    y = np.zeros(2 * n_pairs)
    y[0::2] = 1.0
    return dict(k=P["k"], n1=P["n1"], w0=P["w0"], w=P["w"], v=P["v"], y=y, blocks=[P["users"], P["items"]],
                maps=[np.repeat(ctx, 2).astype(np.int32), mi], plain=None)


def draw(P, t):
    """-> (negatives, attempts, forced) of the problem at epoch t."""
    return sample(P["seed"], t, np.repeat(P["ctx"], P["n_neg"]), P["ptr"], P["rows"], P["M"])


def gradient(s, p, r0, r1, loss):
    """-> (G_w, G_V, e) of the rows [r0, r1) (whole pairs), per block from (P_b, e_b); G_0 = sum e is exactly 0."""
    parts = rref.parts_of(p)
    yh, Q = rref.combine(s, parts, r0, r1)
    e = ref.residuals(yh, p["y"][r0:r1], loss, pairs=True)
    gw, gv = np.zeros_like(s.w), np.zeros_like(s.v)
    for X, mp in parts:
        Pb, eb = np.zeros((X.shape[0], Q.shape[1])), np.zeros(X.shape[0])
        np.add.at(Pb, mp[r0:r1], e[:, None] * Q)
        np.add.at(eb, mp[r0:r1], e)
        gv += (X.T @ Pb).T - s.v * ((X * X).T @ eb)[None, :]
        gw += X.T @ eb
    return gw, gv, e


def step(s, p, r0, r1, eta, reg0, regw, regv, rule):
    """One step of the rows [r0, r1) of the layout `p` under `rule` (its loss and optimizer; pairwise by construction), in place."""
    gw, gv, _ = gradient(s, p, r0, r1, rule.loss)
    b = float(r1 - r0)
    h0, hw, hv = reg0 * s.w0, gw / b + regw * s.w, gv / b + regv * s.v
    if rule.eps is None:
        s.w0, s.w, s.v = s.w0 - eta * h0, s.w - eta * hw, s.v - eta * hv
        return s
    t0, s.n0 = ref.adagrad_rule(np.float64(s.w0), np.float64(s.n0), h0, eta, rule.eps)
    s.w0 = float(t0)
    s.w, s.nw = ref.adagrad_rule(s.w, s.nw, hw, eta, rule.eps)
    s.v, s.nv = ref.adagrad_rule(s.v, s.nv, hv, eta, rule.eps)
    return s


def epochs(s, P, n_epochs, batch_pairs, eta, reg0, regw, regv, rule, t0=0):
    """Epochs t0 .. t0 + n_epochs - 1: resample at t, then every batch of `batch_pairs` pairs in order; -> (s, the last layout)."""
    p = None
    for t in range(t0, t0 + n_epochs):
        p = layout(P, draw(P, t)[0])
        n = len(p["y"])
        br = 2 * batch_pairs if 0 < batch_pairs <= n // 2 else n
        for r0 in range(0, n, br):
            step(s, p, r0, min(n, r0 + br), eta, reg0, regw, regv, rule)
    return s, p


def pair_scores(s, p):
    """-> (mean pair log-loss, concordance) of the layout's pairs at the state's parameters."""
    return ref.pair_scores(rref.predict(s, p), p["y"])


# ---- problems -------------------------------------------------------------------------------------------------------------------

def make_problem(seed, k, n_ctx=40, M=120, n_inter=600, n_neg=1, shuffle=True, positives=None, scale=0.1, user_ids=(0, 100), item_ids=(100, 260)):
    """Users (0-6 nonzeros, ids user_ids) and items (1-8 nonzeros, ids item_ids; row 5 empty when there is one) as relational_ref's
    blocks; `positives`: given, or n_inter distinct (context, row) interactions drawn at random."""
    rng = np.random.default_rng(seed)
    users = rref.random_block(rng, n_ctx, 0, 6, *user_ids)
    items = rref.random_block(rng, M, 1, 8, *item_ids, empty=(5,) if M > 5 else ())
    if positives is None:
        flat = rng.choice(n_ctx * M, size=n_inter, replace=False)
        positives = [np.sort(flat[flat // M == u] % M) for u in range(n_ctx)]
    n1 = item_ids[1]
    ctx, cand, ptr, rows = training_order(positives, M, seed, shuffle)
    prng = np.random.default_rng(seed + 1000)
    return dict(seed=seed, k=k, n1=n1, M=M, n_ctx=n_ctx, n_neg=n_neg, shuffle=shuffle, users=users, items=items, positives=positives,
                ctx=ctx, cand=cand, ptr=ptr, rows=rows, w0=float(prng.normal(0, scale)), w=prng.normal(0, scale, n1),
                v=prng.normal(0, scale, (k, n1)))


def build(fmhip, P, batch_pairs=0, **kw):
    """-> (HipBPR over cached blocks, FMModel at the problem's parameters)."""
    mk = lambda b, name: fmhip.DataSet(b["row_ptr"], b["col"], b["val"], np.zeros(len(b["row_ptr"]) - 1), name=name, batch_rows=0)      # noqa: E731
    bpr = fmhip.HipBPR.run(mk(P["users"], "users"), mk(P["items"], "items"), P["positives"], n_neg=P["n_neg"], batch_pairs=batch_pairs,
                           seed=P["seed"], shuffle=P["shuffle"], **kw)
    fm = fmhip.FMModel(P["n1"] - 1, P["k"])
    fm.w0, fm.w, fm.v = P["w0"], P["w"], P["v"]
    return bpr, fm


# ---- the planted preference task ------------------------------------------------------------------------------------------------------

def planted_task(seed, n_users=30, n_items=80, per_user=16, k_true=4, held=0.2):
    """Two fields: a one-hot user id (ids [0, n_users)) and a one-hot item id (ids [n_users, n_users + n_items)).  A planted FM
    (item bias + <p_u, q_i>) scores every pair; a user's interactions are its `per_user` best items; `held` of them are held out.
    -> dict(users, items, train, held_out: one array of item rows per user; n1)."""
    rng = np.random.default_rng(seed)
    pu, qi, bi = rng.normal(0, 1.0, (n_users, k_true)), rng.normal(0, 1.0, (n_items, k_true)), rng.normal(0, 0.5, n_items)
    score = pu @ qi.T + bi[None, :]
    onehot = lambda n, base: dict(row_ptr=np.arange(n + 1, dtype=np.int64), col=(base + np.arange(n)).astype(np.int32), val=np.ones(n))      # noqa: E731
    train, held_out = [], []
    for u in range(n_users):
        best = rng.permutation(np.argsort(-score[u])[:per_user])
        n_held = int(round(held * per_user))
        held_out.append(np.sort(best[:n_held]))
        train.append(np.sort(best[n_held:]))
    return dict(users=onehot(n_users, 0), items=onehot(n_items, n_users), train=train, held_out=held_out, n1=n_users + n_items)


def ndcg_at(scores, held_out, exclude, k=10):
    """Mean NDCG@k of the held-out rows in every user's ranking of the non-excluded items (best first, ties by ascending row)."""
    total, n = 0.0, 0
    for u, rel in enumerate(held_out):
        if not len(rel):
            continue
        s = np.array(scores[u], np.float64)
        s[np.asarray(exclude[u], np.int64)] = -np.inf
        order = np.lexsort((np.arange(len(s)), -s))
        rank = np.empty(len(s), np.int64)
        rank[order] = np.arange(len(s))
        r = np.sort(rank[np.asarray(rel, np.int64)])
        dcg = (1.0 / np.log2(r[r < k] + 2.0)).sum()
        idcg = (1.0 / np.log2(np.arange(min(len(rel), k)) + 2.0)).sum()
        total += dcg / idcg
        n += 1
    return total / max(n, 1)
