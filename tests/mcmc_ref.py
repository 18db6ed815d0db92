"""The MCMC learner's rule (include/fmhip_mcmc.h) restated in fp64 numpy, in textbook order: one Gibbs sweep draws alpha, the bias, and
then, group by group, lambda_g and mu_g RIGHT BEFORE that group's sweep, one column at a time.  The library hoists the groups' sums to
the epoch's start (nothing writes a group before its own sweep) and draws the whole epoch's noise up front; the counters make both
orders see the same numbers.  Also here: the counter-based generator (Philox4x32-10, u53, Box-Muller, Marsaglia-Tsang), written from
the paper's description independently of csrc/mcmc_rng.h, and the planted rating task the learner is tried on."""
import math

import numpy as np

U = np.uint64
M0, M1, W0, W1, MASK = U(0xD2511F53), U(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85, U(0xFFFFFFFF)
STREAM_COORD, STREAM_W0, STREAM_ALPHA, STREAM_LAMBDA, STREAM_MU = range(5)
PRIORS = dict(alpha_0=1.0, beta_0=1.0, alpha_lambda=1.0, beta_lambda=1.0, gamma_0=1.0, mu_0=0.0)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counters (arrays or ints, broadcast) under key (k0, k1) -> four uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.atleast_1d(np.asarray(c, dtype=np.uint64)) for c in (c0, c1, c2, c3)])
    k0, k1 = int(k0), int(k1)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bits: no overflow
        n0, n2 = (p1 >> U(32)) ^ c1 ^ U(k0), (p0 >> U(32)) ^ c3 ^ U(k1)
        c1, c3, c0, c2 = p1 & MASK, p0 & MASK, n0, n2
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def key_of(seed):
    return seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF


def u53(a, b):
    return (((a << U(32) | b) >> U(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def uniform(seed, index, group, t, stream):
    x = philox(index, group, t, stream, *key_of(seed))
    return u53(x[0], x[1])


def normal(seed, index, group, t, stream):
    x = philox(index, group, t, stream, *key_of(seed))
    return np.sqrt(-2.0 * np.log(u53(x[0], x[1]))) * np.cos(2.0 * np.pi * u53(x[2], x[3]))


def gamma(seed, group, t, stream, shape, rate):
    """Marsaglia-Tsang without the squeeze -> (value, attempts); a shape below 1 draws shape + 1 and scales by u^(1/shape)."""
    a = shape + 1.0 if shape < 1.0 else shape
    d = a - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    j = 0
    while True:
        x, u = float(normal(seed, 2 * j, group, t, stream)[0]), float(uniform(seed, 2 * j + 1, group, t, stream)[0])
        j += 1
        b = 1.0 + c * x
        v = b * b * b
        if v <= 0.0:
            continue
        if math.log(u) < x * x / 2.0 + d - d * v + d * math.log(v):
            out = d * v / rate
            break
    if shape < 1.0:
        out *= float(uniform(seed, 0xFFFFFFFF, group, t, stream)[0]) ** (1.0 / shape)
    return out, j


class Problem:
    """CSR rows + their columns (ascending row order inside a column)."""

    def __init__(self, row_ptr, col, val, y):
        self.row_ptr, self.col, self.val, self.y = np.asarray(row_ptr, np.int64), np.asarray(col, np.int64), np.asarray(val, np.float64), np.asarray(y, np.float64)
        self.n_rows = len(self.row_ptr) - 1
        self.row_of = np.repeat(np.arange(self.n_rows), np.diff(self.row_ptr))
        order = np.lexsort((self.row_of, self.col))
        cs, self.crow, self.cval = self.col[order], self.row_of[order], self.val[order]
        self.feat, start = np.unique(cs, return_index=True)
        self.cptr = np.append(start, len(cs))


def predict(w0, w, v, p):
    """FMModel.predict of every row of Problem p (v: [k, n1])."""
    out = w0 + np.bincount(p.row_of, w[p.col] * p.val, p.n_rows)
    for f in range(v.shape[0]):
        t = v[f, p.col] * p.val
        s = np.bincount(p.row_of, t, p.n_rows)
        out += 0.5 * (s * s - np.bincount(p.row_of, t * t, p.n_rows))
    return out


class State:
    def __init__(self, w0, w, v, init_lambda=1.0):
        self.w0, self.w, self.v = float(w0), np.array(w, np.float64), np.array(v, np.float64)
        k1 = self.v.shape[0] + 1
        self.alpha, self.lam, self.mu, self.t = 1.0, np.full(k1, float(init_lambda)), np.zeros(k1), 0


def conditional(theta, alpha, lam, mu, seh, shs, z, sample):
    prec = lam + alpha * shs
    mean = -(alpha * (seh - theta * shs) - mu * lam) / prec
    return mean + z / math.sqrt(prec) if sample else mean


def updatable(new, old):
    return math.isfinite(new) and new != old


def epoch(st, p, seed=0, sample=True, reg0=0.0, priors=PRIORS):
    """One Gibbs sweep of State st over Problem p, in place -> the epoch's starting sum of squared residuals."""
    pr = dict(PRIORS, **priors)
    t, n1 = st.t, len(st.w)
    num_attribute = n1 - 1
    e = predict(st.w0, st.w, st.v, p) - p.y
    sse = float(e @ e)
    if sample:
        st.alpha = gamma(seed, 0, t, STREAM_ALPHA, (pr["alpha_0"] + p.n_rows) / 2.0, (pr["beta_0"] + sse) / 2.0)[0]
    new = conditional(st.w0, st.alpha, reg0, 0.0, float(e.sum()), float(p.n_rows), float(normal(seed, 0, 0, t, STREAM_W0)[0]), sample)
    if updatable(new, st.w0):
        st.w0 = new
    e = predict(st.w0, st.w, st.v, p) - p.y
    slots = np.flatnonzero(p.feat < num_attribute)            # quirk Q1: slot n is never trained
    T = p.feat[slots]
    m = len(T)
    for g in range(st.v.shape[0] + 1):
        theta = st.w if g == 0 else st.v[g - 1]
        if sample:
            dev = theta[T] - st.mu[g]
            st.lam[g] = gamma(seed, g, t, STREAM_LAMBDA, (pr["alpha_lambda"] + m + 1.0) / 2.0,
                              (pr["beta_lambda"] + float(dev @ dev) + pr["gamma_0"] * (st.mu[g] - pr["mu_0"]) ** 2) / 2.0)[0]
            wgt = m + pr["gamma_0"]
            st.mu[g] = (float(theta[T].sum()) + pr["gamma_0"] * pr["mu_0"]) / wgt + float(normal(seed, 0, g, t, STREAM_MU)[0]) / math.sqrt(wgt * st.lam[g])
        q = np.bincount(p.row_of, theta[p.col] * p.val, p.n_rows) if g else None
        z = normal(seed, T, g, t, STREAM_COORD) if m else np.zeros(0)
        for j, s in enumerate(slots):
            i, rows, x = int(p.feat[s]), p.crow[p.cptr[s]:p.cptr[s + 1]], p.cval[p.cptr[s]:p.cptr[s + 1]]
            th = float(theta[i])
            h = x * q[rows] - x * x * th if g else x
            new = conditional(th, st.alpha, st.lam[g], st.mu[g], float(e[rows] @ h), float(h @ h), float(z[j]), sample)
            if updatable(new, th):
                d = new - th
                e[rows] += h * d
                if g:
                    q[rows] += x * d
                theta[i] = new
    st.t += 1
    return sse


def planted_task(seed, n_train=600, n_test=300, sizes=(30, 40), k=2, sigma=0.3):
    """Two one-hot fields, y = 3.5 + w_u + w_i + <v_u, v_i> + N(0, sigma^2) -> (train, test) dicts of row_ptr, col, val, y, n1."""
    rng = np.random.default_rng(seed)
    n1 = sum(sizes) + 1                                        # (one spare slot: quirk Q1's untrained last id)
    w = rng.normal(0, 0.5, n1)
    v = rng.normal(0, 0.7, (k, n1))
    out = []
    for n in (n_train, n_test):
        u, i = rng.integers(0, sizes[0], n), sizes[0] + rng.integers(0, sizes[1], n)
        y = 3.5 + w[u] + w[i] + (v[:, u] * v[:, i]).sum(0) + rng.normal(0, sigma, n)
        out.append(dict(row_ptr=np.arange(0, 2 * n + 1, 2, dtype=np.int64), col=np.stack([u, i], 1).reshape(-1).astype(np.int32),
                        val=np.ones(2 * n), y=y, n1=n1))
    return out


def rmse(yhat, y):
    return float(np.sqrt(np.mean((yhat - y) ** 2)))
