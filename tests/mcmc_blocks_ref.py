"""The MCMC learner's block-structure sweep (include/fmhip_mcmc_relational.h) restated in fp64 numpy BY BLOCK CACHES: the residuals from
the blocks' yhat_p and q_p, per (part, parameter group) the caches E, A, B, C over the data rows that map to a block row, the column
step from them, the scatter back to e and Q_f — every element-wise operation in the header's order, a column's sum by numpy's dot.  On
mcmc_ref's philox / gamma / normal / conditional and probit_ref's truncated normal, with the flat sweep's counters: a run with seed s
draws what mcmc_ref / mcmc_groups_ref draw on the expanded rows.  Also here: the small relational problem the learner is tried on (a
user block with two rows nobody references and a feature that lives only there, an item block with one hot item, a plain part) and its
expansion to mcmc_ref.Problem.  Neither twin is the code under test; test_host_mcmc_relational.py pins this one to the flat ones."""
import math

import numpy as np

import mcmc_ref as R
import probit_ref as PR


class Block(R.Problem):
    """A part: the block's rows (labels of zero) and the mapping (None: the plain part, the identity)."""

    def __init__(self, row_ptr, col, val, mapping=None):
        super().__init__(row_ptr, col, val, np.zeros(len(row_ptr) - 1))
        self.mapping = None if mapping is None else np.asarray(mapping, np.int64)

    def rows_of(self, n_rows):
        return np.arange(n_rows) if self.mapping is None else self.mapping


class Relational:
    def __init__(self, y, parts):
        self.y, self.parts, self.n_rows = np.asarray(y, np.float64), list(parts), len(y)
        lo = [int(p.feat.min()) if len(p.feat) else 2 ** 31 for p in self.parts]
        self.order = sorted(range(len(self.parts)), key=lambda p: lo[p])          # the walk: ascending id ranges

    def expand(self):
        """-> mcmc_ref.Problem of the flat rows: part 0's entries of the row's block row, then part 1's, ..."""
        cols, vals, ptr = [], [], [0]
        for r in range(self.n_rows):
            for p in self.parts:
                j = p.rows_of(self.n_rows)[r]
                cols.append(p.col[p.row_ptr[j]:p.row_ptr[j + 1]])
                vals.append(p.val[p.row_ptr[j]:p.row_ptr[j + 1]])
            ptr.append(ptr[-1] + sum(len(c) for c in cols[-len(self.parts):]))
        return R.Problem(ptr, np.concatenate(cols), np.concatenate(vals), self.y)


class State:
    def __init__(self, w0, w, v, n_groups=1, init_lambda=1.0):
        self.w0, self.w, self.v = float(w0), np.array(w, np.float64), np.array(v, np.float64)
        k1 = self.v.shape[0] + 1
        self.G = int(n_groups)
        self.alpha, self.lam, self.mu, self.t = 1.0, np.full((k1, self.G), float(init_lambda)), np.zeros((k1, self.G)), 0
        self.ystar = None


def counts(rp, part):
    return np.bincount(part.rows_of(rp.n_rows), minlength=part.n_rows).astype(np.float64)


def trained(rp, part, num_attribute):
    """-> the part's column slots in T: id < num_attribute and an entry in a block row some data row maps to."""
    n = counts(rp, part)
    return np.array([s for s in range(len(part.feat)) if part.feat[s] < num_attribute and (n[part.crow[part.cptr[s]:part.cptr[s + 1]]] > 0).any()], np.int64)


def group_counts(rp, num_attribute):
    return np.array([len(trained(rp, p, num_attribute)) for p in rp.parts])


def residual_parts(st, rp):
    """-> (yhat [N], Q [k, N], q_p per part [k, J_p]) by the header's residual rule."""
    k = st.v.shape[0]
    yhat = np.full(rp.n_rows, st.w0)
    qs, js = [], []
    for p in rp.parts:
        j = p.rows_of(rp.n_rows)
        yhat = yhat + (R.predict(st.w0, st.w, st.v, p)[j] - st.w0)
        qs.append(np.stack([np.bincount(p.row_of, st.v[f, p.col] * p.val, p.n_rows) for f in range(k)]) if k else np.zeros((0, p.n_rows)))
        js.append(j)
    Q = np.zeros((k, rp.n_rows))
    for f in range(k):
        run, cross = qs[0][f, js[0]].copy(), np.zeros(rp.n_rows)
        for q, j in zip(qs[1:], js[1:]):
            cross = cross + run * q[f, j]
            run = run + q[f, j]
        yhat = yhat + cross
        Q[f] = run
    return yhat, Q, qs


def predict(st, rp):
    return residual_parts(st, rp)[0]


def epoch(st, rp, seed=0, sample=True, reg0=0.0, priors=R.PRIORS, task="regression"):
    """One block-structure Gibbs sweep of State st over Relational rp, in place -> the epoch's starting sum of squared residuals.
    st.G = 1: ungrouped; st.G = len(rp.parts): a part is an attribute group."""
    pr = dict(R.PRIORS, **priors)
    t, N = st.t, rp.n_rows
    num_attribute = len(st.w) - 1
    grouped = st.G > 1
    yhat, Q, qs = residual_parts(st, rp)
    if task == "classification":
        s = np.where(rp.y > 0, 1.0, -1.0)
        if t == 0:
            y = s.copy()
        else:
            a = -s * yhat
            z = PR.truncated_normal(seed, np.arange(N), t, a)[0] if sample else PR.truncated_mean(a)
            y = yhat + s * z
        st.ystar = y
    else:
        y = rp.y
    e = yhat - y
    sse = float(e @ e)
    if sample and task != "classification":
        st.alpha = R.gamma(seed, 0, t, R.STREAM_ALPHA, (pr["alpha_0"] + N) / 2.0, (pr["beta_0"] + sse) / 2.0)[0]
    new = R.conditional(st.w0, st.alpha, reg0, 0.0, float(e.sum()), float(N), float(R.normal(seed, 0, 0, t, R.STREAM_W0)[0]), sample)
    if R.updatable(new, st.w0):
        st.w0 = new
    e = residual_parts(st, rp)[0] - y
    slots = [trained(rp, p, num_attribute) for p in rp.parts]
    ns = [counts(rp, p) for p in rp.parts]
    for g in range(st.v.shape[0] + 1):
        theta = st.w if g == 0 else st.v[g - 1]
        if sample:
            sets = [[p] for p in range(len(rp.parts))] if grouped else [rp.order]
            for a, members in enumerate(sets):
                T = np.concatenate([rp.parts[p].feat[slots[p]] for p in members]).astype(np.int64)
                m, word = len(T), g + (a << 16)
                dev = theta[T] - st.mu[g, a]
                st.lam[g, a] = R.gamma(seed, word, t, R.STREAM_LAMBDA, (pr["alpha_lambda"] + m + 1.0) / 2.0,
                                       (pr["beta_lambda"] + float(dev @ dev) + pr["gamma_0"] * (st.mu[g, a] - pr["mu_0"]) ** 2) / 2.0)[0]
                wgt = m + pr["gamma_0"]
                st.mu[g, a] = ((float(theta[T].sum()) + pr["gamma_0"] * pr["mu_0"]) / wgt
                               + float(R.normal(seed, 0, word, t, R.STREAM_MU)[0]) / math.sqrt(wgt * st.lam[g, a]))
        for p in rp.order:
            part, a = rp.parts[p], (p if grouped else 0)
            jr, n = part.rows_of(N), ns[p]
            T = part.feat[slots[p]]
            z = R.normal(seed, T, g, t, R.STREAM_COORD) if len(T) else np.zeros(0)
            J = part.n_rows
            # the caches, once per (part, group)
            E = np.bincount(jr, e, J)
            S2 = np.zeros(J)
            if g:
                qp = qs[p][g - 1]
                qr = Q[g - 1] - qp[jr]
                A, B, C, S1 = np.bincount(jr, qr, J), np.bincount(jr, qr * qr, J), np.bincount(jr, e * qr, J), np.zeros(J)
            for zi, sl in enumerate(slots[p]):
                i, rows, x = int(part.feat[sl]), part.crow[part.cptr[sl]:part.cptr[sl + 1]], part.cval[part.cptr[sl]:part.cptr[sl + 1]]
                th = float(theta[i])
                if g:
                    u = qp[rows] - x * th
                    shs = float(((x * x) * ((n[rows] * (u * u) + (2.0 * u) * A[rows]) + B[rows])).sum())
                    seh = float((x * (u * E[rows] + C[rows])).sum())
                else:
                    shs, seh = float(((x * x) * n[rows]).sum()), float((x * E[rows]).sum())
                new = R.conditional(th, st.alpha, st.lam[g, a], st.mu[g, a], seh, shs, float(z[zi]), sample)
                if R.updatable(new, th):
                    xd = x * (new - th)
                    if g:
                        E[rows] += xd * (n[rows] * u + A[rows])
                        C[rows] += xd * (u * A[rows] + B[rows])
                        S1[rows] += xd * u
                        S2[rows] += xd
                        qp[rows] += xd
                    else:
                        E[rows] += n[rows] * xd
                        S2[rows] += xd
                    theta[i] = new
            # the scatter
            if g:
                e += S1[jr] + S2[jr] * qr
                Q[g - 1] += S2[jr]
            else:
                e += S2[jr]
    st.t += 1
    return sse


# ---- the problem ------------------------------------------------------------------------------------------------------------------

USERS, ITEMS, HISTORY, GENRES, PLAIN = 40, 25, 12, 6, 4


def base_problem(seed, n_rows=300, n_test=120, k=3, classification=False):
    """Ids contiguous per part: users [0, 40), history [40, 52), the feature that lives only in the two users nobody references 52,
    items [53, 78), genres [78, 84), plain [84, 88), and 88 = num_attribute (quirk Q1's slot, stored in one plain row).  Users 38 and
    39 are referenced by nobody; item 3 by ~45% of the rows (n_rows = 700: a list of more than 256 rows, summed in chunks).
    -> dict(train, test: Relational; n1, k, w0, w, v)."""
    rng = np.random.default_rng(seed)
    lonely = USERS + HISTORY
    item0 = lonely + 1
    genre0, plain0 = item0 + ITEMS, item0 + ITEMS + GENRES
    n1 = plain0 + PLAIN + 1
    ucol, uval, uptr = [], [], [0]
    for u in range(USERS):
        hist = np.sort(rng.choice(HISTORY, rng.integers(2, 5), replace=False)) + USERS
        c = np.concatenate([[u], hist, [lonely] if u >= USERS - 2 else []]).astype(np.int64)
        ucol.append(c)
        uval.append(np.concatenate([[1.0], rng.uniform(0.2, 1.0, len(c) - 1)]))
        uptr.append(uptr[-1] + len(c))
    icol, ival, iptr = [], [], [0]
    for i in range(ITEMS):
        gen = np.sort(rng.choice(GENRES, rng.integers(1, 3), replace=False)) + genre0
        icol.append(np.concatenate([[item0 + i], gen]))
        ival.append(np.concatenate([[1.0], rng.uniform(0.5, 1.0, len(gen))]))
        iptr.append(iptr[-1] + len(gen) + 1)
    ublock = (np.array(uptr), np.concatenate(ucol), np.concatenate(uval))
    iblock = (np.array(iptr), np.concatenate(icol), np.concatenate(ival))
    w_true, v_true = rng.normal(0, 0.5, n1), rng.normal(0, 0.6, (2, n1))
    out = {}
    for name, n in (("train", n_rows), ("test", n_test)):
        umap = rng.integers(0, USERS - 2, n)
        imap = np.where(rng.random(n) < 0.45, 3, rng.integers(0, ITEMS, n))
        pcol, pval, pptr = [], [], [0]
        for r in range(n):
            keep = np.flatnonzero(rng.random(PLAIN) < 0.8)
            c, x = keep + plain0, rng.normal(0, 1, len(keep))
            if name == "train" and r == 5:
                c, x = np.append(c, n1 - 1), np.append(x, 0.7)
            pcol.append(c)
            pval.append(x)
            pptr.append(pptr[-1] + len(c))
        parts = [Block(*ublock, mapping=umap), Block(*iblock, mapping=imap), Block(np.array(pptr), np.concatenate(pcol), np.concatenate(pval))]
        rp = Relational(np.zeros(n), parts)
        flat = rp.expand()
        truth = R.State(3.0, w_true, v_true)
        y = R.predict(truth.w0, truth.w, truth.v, flat) + rng.normal(0, 0.3, n)
        out[name] = (rp, y)
    cut = float(np.median(out["train"][1]))
    for name in ("train", "test"):
        rp, y = out[name]
        rp.y = (y > cut).astype(np.float64) if classification else y
        out[name] = rp
    out.update(n1=n1, k=k, w0=0.1, w=rng.normal(0, 0.1, n1), v=rng.normal(0, 0.1, (k, n1)), lonely=lonely)
    return out


def distance(a, b):
    """The largest relative distance between two arrays (or scalars): max |a - b| / max(|b|, 1e-300) elementwise, over the entries."""
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300))) if len(a) else 0.0
