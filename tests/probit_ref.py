"""The MCMC learner's classification rule (include/fmhip_mcmc_task.h) restated in fp64 numpy on top of mcmc_ref.py: the truncated-normal
draw by rejection from stream 5 (vectorised over the rows; it returns the attempt counts and the SMALLEST MARGIN by which any accept /
reject decision was taken — |z - a| on the normal branch, |u2 - rho| on the exponential one — so that a test can tell whether a
last-bit difference in yhat could have flipped a decision), its expectation, and the Gibbs sweep on the latent targets with alpha kept
what the state holds.  The sweep is mcmc_ref.epoch's, textbook order, with y* where that reads y and without alpha's draw."""
import math

import numpy as np

import mcmc_ref as R

STREAM_TARGET = 5
MAX_ATTEMPTS = 64
_erfc = np.vectorize(math.erfc, otypes=[np.float64])


def normal_cdf(x):
    return 0.5 * _erfc(-np.asarray(x, np.float64) / math.sqrt(2.0))


def truncated_normal(seed, rows, t, a):
    """z ~ N(0,1) given z > a, one per row (counter (row, attempt, t, 5)) -> (z, attempts, smallest decision margin)."""
    rows, a = np.atleast_1d(np.asarray(rows, np.uint64)), np.atleast_1d(np.asarray(a, np.float64))
    z, attempts = np.zeros(len(a)), np.zeros(len(a), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        lam = (a + np.sqrt(a * a + 4.0)) / 2.0
    todo, margin = np.arange(len(a)), np.inf
    for j in range(MAX_ATTEMPTS):
        if not len(todo):
            break
        x = R.philox(rows[todo], j, t, STREAM_TARGET, *R.key_of(seed))
        u1, u2 = R.u53(x[0], x[1]), R.u53(x[2], x[3])
        at, left = a[todo], a[todo] <= 0.0
        with np.errstate(invalid="ignore", over="ignore"):
            zn = np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)
            ze = at - np.log(u1) / lam[todo]
            d = ze - lam[todo]
            rho = np.exp(-0.5 * (d * d))
        ok = np.where(left, zn > at, u2 <= rho)
        m = np.where(left, np.abs(zn - at), np.abs(u2 - rho))
        if len(m) and np.isfinite(m).any():
            margin = min(margin, float(np.nanmin(m)))
        prop = np.where(left, zn, ze)
        if j == MAX_ATTEMPTS - 1:
            prop = np.where(left & ~ok, np.abs(zn), prop)
            ok = np.ones(len(todo), bool)
        z[todo], attempts[todo] = prop, j + 1
        todo = todo[~ok]
    return z, attempts, margin


def truncated_mean(a):
    """E[z | z > a] = phi(a) / Q(a); a + 1 / a past a = 30."""
    a = np.atleast_1d(np.asarray(a, np.float64))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = np.exp(-0.5 * (a * a)) * 0.3989422804014327 / (0.5 * _erfc(a / math.sqrt(2.0)))
        return np.where(a > 30.0, a + 1.0 / a, q)


def latent_targets(st, p, seed=0, sample=True):
    """Step 2 of the rule under the state's parameters -> (y*, yhat, s, z, attempts, margin); t = 0: y* = s, no draw."""
    yhat = R.predict(st.w0, st.w, st.v, p)
    s = np.where(p.y > 0, 1.0, -1.0)
    if st.t == 0:
        return s.copy(), yhat, s, None, None, np.inf
    a = -s * yhat
    if sample:
        z, attempts, margin = truncated_normal(seed, np.arange(p.n_rows), st.t, a)
    else:
        z, attempts, margin = truncated_mean(a), None, np.inf
    return yhat + s * z, yhat, s, z, attempts, margin


def epoch(st, p, seed=0, sample=True, reg0=0.0, priors=R.PRIORS):
    """One Gibbs sweep of a classification handle, in place -> dict(sse of the latent residuals, ystar, yhat, s, z, attempts, margin)."""
    pr = dict(R.PRIORS, **priors)
    t, n1 = st.t, len(st.w)
    ystar, yhat, s, z_t, attempts, margin = latent_targets(st, p, seed, sample)
    e = yhat - ystar
    sse = float(e @ e)
    new = R.conditional(st.w0, st.alpha, reg0, 0.0, float(e.sum()), float(p.n_rows), float(R.normal(seed, 0, 0, t, R.STREAM_W0)[0]), sample)
    if R.updatable(new, st.w0):
        st.w0 = new
    e = R.predict(st.w0, st.w, st.v, p) - ystar
    slots = np.flatnonzero(p.feat < n1 - 1)
    T = p.feat[slots]
    m = len(T)
    for g in range(st.v.shape[0] + 1):
        theta = st.w if g == 0 else st.v[g - 1]
        if sample:
            dev = theta[T] - st.mu[g]
            st.lam[g] = R.gamma(seed, g, t, R.STREAM_LAMBDA, (pr["alpha_lambda"] + m + 1.0) / 2.0,
                                (pr["beta_lambda"] + float(dev @ dev) + pr["gamma_0"] * (st.mu[g] - pr["mu_0"]) ** 2) / 2.0)[0]
            wgt = m + pr["gamma_0"]
            st.mu[g] = (float(theta[T].sum()) + pr["gamma_0"] * pr["mu_0"]) / wgt + float(R.normal(seed, 0, g, t, R.STREAM_MU)[0]) / math.sqrt(wgt * st.lam[g])
        q = np.bincount(p.row_of, theta[p.col] * p.val, p.n_rows) if g else None
        z = R.normal(seed, T, g, t, R.STREAM_COORD) if m else np.zeros(0)
        for j, sl in enumerate(slots):
            i, rows, x = int(p.feat[sl]), p.crow[p.cptr[sl]:p.cptr[sl + 1]], p.cval[p.cptr[sl]:p.cptr[sl + 1]]
            th = float(theta[i])
            h = x * q[rows] - x * x * th if g else x
            new = R.conditional(th, st.alpha, st.lam[g], st.mu[g], float(e[rows] @ h), float(h @ h), float(z[j]), sample)
            if R.updatable(new, th):
                d = new - th
                e[rows] += h * d
                if g:
                    q[rows] += x * d
                theta[i] = new
    st.t += 1
    return dict(sse=sse, ystar=ystar, yhat=yhat, s=s, z=z_t, attempts=attempts, margin=margin)


def logloss(p, y):
    """Mean log-loss of probabilities p against the classes [y > 0] (p clipped away from 0 and 1 by 1e-15)."""
    p, t = np.clip(np.asarray(p, np.float64), 1e-15, 1.0 - 1e-15), np.asarray(y) > 0
    return float(-np.mean(np.where(t, np.log(p), np.log1p(-p)))) if len(p) else 0.0


def accuracy(p, y):
    return float(np.mean((np.asarray(p) > 0.5) == (np.asarray(y) > 0))) if len(p) else 0.0


def median_cut(tr, te=None):
    """Labels cut at the train median -> 1.0 above it, 0.0 otherwise (copies of the dicts)."""
    cut = float(np.median(tr["y"]))
    out = [dict(d, y=(d["y"] > cut).astype(np.float64)) for d in ((tr,) if te is None else (tr, te))]
    return out[0] if te is None else out
