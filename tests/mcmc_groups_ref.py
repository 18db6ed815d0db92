"""The MCMC learner with attribute groups (include/fmhip_mcmc_groups.h) restated in fp64 numpy: mcmc_ref.epoch with step 4 changed —
lambda and mu per (parameter group g, attribute group a), drawn for a = 0 .. G-1 right before group g's sweep, every column's
conditional taking its own group's pair — on mcmc_ref's philox / gamma / normal / conditional.  The hyper-parameter draws put
g + (a << 16) into the counter's group word, so G = 1 is mcmc_ref.epoch in every random number.  `targets` composes it with
probit_ref: a classification handle trains on latent targets and does not draw alpha."""
import math

import numpy as np

import mcmc_ref as R


class State:
    def __init__(self, w0, w, v, group, n_groups, init_lambda=1.0):
        self.w0, self.w, self.v = float(w0), np.array(w, np.float64), np.array(v, np.float64)
        k1 = self.v.shape[0] + 1
        self.group, self.G = np.asarray(group, np.int64), int(n_groups)
        self.alpha, self.lam, self.mu, self.t = 1.0, np.full((k1, self.G), float(init_lambda)), np.zeros((k1, self.G)), 0


def trained(st, p):
    """-> (column slots of the trained features, their ids): ids < num_attribute (quirk Q1: slot n is never trained)."""
    slots = np.flatnonzero(p.feat < len(st.w) - 1)
    return slots, p.feat[slots]


def group_counts(st, p):
    return np.bincount(st.group[trained(st, p)[1]], minlength=st.G)


def epoch(st, p, seed=0, sample=True, reg0=0.0, priors=R.PRIORS, y=None, draw_alpha=True):
    """One Gibbs sweep of State st over Problem p, in place -> the epoch's starting sum of squared residuals.  y: the targets the
    epoch trains on (default: p.y); draw_alpha False: alpha stays (the probit link)."""
    pr = dict(R.PRIORS, **priors)
    t = st.t
    y = p.y if y is None else y
    e = R.predict(st.w0, st.w, st.v, p) - y
    sse = float(e @ e)
    if sample and draw_alpha:
        st.alpha = R.gamma(seed, 0, t, R.STREAM_ALPHA, (pr["alpha_0"] + p.n_rows) / 2.0, (pr["beta_0"] + sse) / 2.0)[0]
    new = R.conditional(st.w0, st.alpha, reg0, 0.0, float(e.sum()), float(p.n_rows), float(R.normal(seed, 0, 0, t, R.STREAM_W0)[0]), sample)
    if R.updatable(new, st.w0):
        st.w0 = new
    e = R.predict(st.w0, st.w, st.v, p) - y
    slots, T = trained(st, p)
    for g in range(st.v.shape[0] + 1):
        theta = st.w if g == 0 else st.v[g - 1]
        if sample:
            for a in range(st.G):
                Ta = T[st.group[T] == a]
                m, word = len(Ta), g + (a << 16)
                dev = theta[Ta] - st.mu[g, a]
                st.lam[g, a] = R.gamma(seed, word, t, R.STREAM_LAMBDA, (pr["alpha_lambda"] + m + 1.0) / 2.0,
                                       (pr["beta_lambda"] + float(dev @ dev) + pr["gamma_0"] * (st.mu[g, a] - pr["mu_0"]) ** 2) / 2.0)[0]
                wgt = m + pr["gamma_0"]
                st.mu[g, a] = ((float(theta[Ta].sum()) + pr["gamma_0"] * pr["mu_0"]) / wgt
                               + float(R.normal(seed, 0, word, t, R.STREAM_MU)[0]) / math.sqrt(wgt * st.lam[g, a]))
        q = np.bincount(p.row_of, theta[p.col] * p.val, p.n_rows) if g else None
        z = R.normal(seed, T, g, t, R.STREAM_COORD) if len(T) else np.zeros(0)
        for j, s in enumerate(slots):
            i, rows, x = int(p.feat[s]), p.crow[p.cptr[s]:p.cptr[s + 1]], p.cval[p.cptr[s]:p.cptr[s + 1]]
            a = st.group[i]
            th = float(theta[i])
            h = x * q[rows] - x * x * th if g else x
            new = R.conditional(th, st.alpha, st.lam[g, a], st.mu[g, a], float(e[rows] @ h), float(h @ h), float(z[j]), sample)
            if R.updatable(new, th):
                d = new - th
                e[rows] += h * d
                if g:
                    q[rows] += x * d
                theta[i] = new
    st.t += 1
    return sse


def planted_task(seed, n_train=600, n_test=300, sizes=(30, 40), k=2, sigma=0.3):
    """Two one-hot fields whose linear weights live on different scales: y = 3.5 + w_u + w_i + <v_u, v_i> + N(0, sigma^2) with user
    w ~ N(0, 2^2), item w ~ N(0, 0.1^2), v ~ N(0, 1) -> (train, test) dicts of row_ptr, col, val, y, n1 (one spare slot: quirk Q1)."""
    rng = np.random.default_rng(seed)
    n1 = sum(sizes) + 1
    w = np.concatenate([rng.normal(0, 2.0, sizes[0]), rng.normal(0, 0.1, sizes[1]), [0.0]])
    v = rng.normal(0, 1.0, (k, n1))
    out = []
    for n in (n_train, n_test):
        u, i = rng.integers(0, sizes[0], n), sizes[0] + rng.integers(0, sizes[1], n)
        y = 3.5 + w[u] + w[i] + (v[:, u] * v[:, i]).sum(0) + rng.normal(0, sigma, n)
        out.append(dict(row_ptr=np.arange(0, 2 * n + 1, 2, dtype=np.int64), col=np.stack([u, i], 1).reshape(-1).astype(np.int32),
                        val=np.ones(2 * n), y=y, n1=n1))
    return out
