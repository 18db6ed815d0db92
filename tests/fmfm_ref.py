"""The fp64 twin of the field-matrixed FM (include/fmhip_fmfm.h), from the naive pairwise definition: a double loop over the entries
a < b of different fields, term x_a x_b v_a^T M[f_a][f_b] v_b, nothing clever.  Rows are lists of (field, feature, value), as ffm_ref's;
m is (F, F, k, k) with m[g][f] = m[f][g].T and zero diagonal blocks."""
import numpy as np

from ffm_ref import P_BATCH, P_EPOCHS, P_ETA, P_K, P_REGV, planted, random_rows  # noqa: F401


def identity(F, k):
    m = np.zeros((F, F, k, k))
    m[:] = np.eye(k)
    m[np.arange(F), np.arange(F)] = 0.0
    return m


class State:
    def __init__(self, w0, w, v, m, init=None):
        self.w0, self.w, self.v, self.m = float(w0), np.array(w, np.float64), np.array(v, np.float64), np.array(m, np.float64)
        if init is not None:          # AdaGrad's accumulators
            self.n0, self.nw, self.nv, self.nm = float(init), np.full_like(self.w, init), np.full_like(self.v, init), np.full_like(self.m, init)


def predict_row(s, row):
    """(yhat, sum of |terms|) of one row."""
    yh, mag = s.w0, abs(s.w0)
    for f, i, x in row:
        yh += s.w[i] * x
        mag += abs(s.w[i] * x)
    for a in range(len(row)):
        for b in range(a + 1, len(row)):
            (fa, ia, xa), (fb, ib, xb) = row[a], row[b]
            if fa != fb:
                t = xa * xb * float(s.v[ia] @ s.m[fa, fb] @ s.v[ib])
                yh += t
                mag += abs(t)
    return yh, mag


def predict(s, rows):
    out = np.array([predict_row(s, r) for r in rows], np.float64).reshape(-1, 2)
    return out[:, 0], out[:, 1]


def logloss(s, rows, y):
    yh = predict(s, rows)[0]
    return float(np.mean(np.maximum(yh, 0.0) - (y > 0) * yh + np.log1p(np.exp(-np.abs(yh)))))


def touched(rows, n1):
    """[n1] bool: the features a batch holds."""
    t = np.zeros(n1, bool)
    for row in rows:
        for _, i, _ in row:
            t[i] = True
    return t


def step(s, rows, y, eta, reg0, regw, regv, regm=0.0, loss="squared", optimizer="sgd", eps=1e-10, linear=True, field_matrices=True):
    """One mini-batch step in place -> touched(rows)."""
    B = len(rows)
    yh, y = predict(s, rows)[0], np.asarray(y, np.float64)
    e = yh - y if loss == "squared" else 1.0 / (1.0 + np.exp(-yh)) - (y > 0)
    gv, gw, gm = np.zeros_like(s.v), np.zeros_like(s.w), np.zeros_like(s.m)
    for r, row in enumerate(rows):
        for a, (fa, ia, xa) in enumerate(row):
            gw[ia] += e[r] * xa / B
            for b in range(a + 1, len(row)):
                fb, ib, xb = row[b]
                if fa == fb:
                    continue
                c = e[r] * xa * xb / B
                gv[ia] += c * (s.m[fa, fb] @ s.v[ib])
                gv[ib] += c * (s.m[fb, fa] @ s.v[ia])
                d = c * np.outer(s.v[ia], s.v[ib])          # one parameter block for the unordered pair
                gm[fa, fb] += d
                gm[fb, fa] += d.T
    g0 = e.sum() / B
    t = touched(rows, len(s.w))

    def upd(theta, n, g, mask):
        if optimizer == "sgd":
            return np.where(mask, theta - eta * g, theta), n
        n2 = n + g * g
        return np.where(mask, theta - eta * g / (np.sqrt(n2) + eps), theta), np.where(mask, n2, n)

    ada = optimizer == "adagrad"
    nv, nw, n0, nm = (s.nv, s.nw, s.n0, s.nm) if ada else (None,) * 4
    s.v, nv = upd(s.v, nv, gv + regv * s.v, t[:, None])
    if linear:
        s.w, nw = upd(s.w, nw, gw + regw * s.w, t)
        w0, n0 = upd(s.w0, n0, g0 + reg0 * s.w0, True)
        s.w0 = float(w0)
    if field_matrices:
        F = s.m.shape[0]
        s.m, nm = upd(s.m, nm, gm + regm * s.m, ~np.eye(F, dtype=bool)[:, :, None, None])          # a diagonal block is no parameter
    if ada:
        s.nv, s.nw, s.n0, s.nm = nv, nw, float(n0), nm
    return t


def epoch(s, rows, y, batch_rows, order=None, **kw):
    n = len(rows)
    br = n if batch_rows <= 0 else batch_rows
    starts = list(range(0, n, br))
    for j in (range(len(starts)) if order is None else order):
        lo = starts[j]
        step(s, rows[lo:lo + br], y[lo:lo + br], **kw)
    return s


def planted_init(t, F):
    v = np.random.default_rng(t["seed"] + 1).random((t["n1"], P_K)) / np.sqrt(P_K)
    return State(0.0, np.zeros(t["n1"]), v, identity(F, P_K), init=1.0)


def run_planted(t, F, field_matrices=True, epochs=P_EPOCHS):
    """Trains the twin on ffm_ref.planted() -> (state, train log-loss, test log-loss); field_matrices=False: the plain FM (M = I, frozen)."""
    (xtr, ytr), (xte, yte) = t["train"], t["test"]
    s = planted_init(t, F)
    for _ in range(epochs):
        epoch(s, xtr, ytr, P_BATCH, eta=P_ETA, reg0=0.0, regw=0.0, regv=P_REGV, loss="logistic", optimizer="adagrad", field_matrices=field_matrices)
    return s, logloss(s, xtr, ytr), logloss(s, xte, yte)
