"""The fp64 twin of DeepFM (include/fmhip_deepfm.h), written as the header states it: the plain FM over a row's entries as a double loop
over a < b, the MLP as one matmul a layer, the chain rule a layer at a time.  Rows are lists of (field, feature, value), as ffm_ref's;
layers is a list of (W_l [n_{l-1}, n_l], b_l [n_l]) with n_0 = F k, u is [n_L]."""
import copy

import numpy as np

from ffm_ref import P_BATCH, P_EPOCHS, P_ETA, P_FIELDS, P_K, P_REGV, planted, random_rows  # noqa: F401


class State:
    def __init__(self, w0, w, v, layers, u, init=None):
        self.w0, self.w, self.v, self.u = float(w0), np.array(w, np.float64), np.array(v, np.float64), np.array(u, np.float64)
        self.layers = [(np.array(W, np.float64), np.array(b, np.float64)) for W, b in layers]
        if init is not None:          # AdaGrad's accumulators
            self.n0, self.nw, self.nv, self.nu = float(init), np.full_like(self.w, init), np.full_like(self.v, init), np.full_like(self.u, init)
            self.nlayers = [(np.full_like(W, init), np.full_like(b, init)) for W, b in self.layers]


def dense(rng, F, k, hidden):
    """He-uniform layers and u, zero biases: (layers, u)."""
    layers, fan = [], F * k
    for n in hidden:
        layers.append((rng.uniform(-1, 1, (fan, n)) * np.sqrt(6.0 / fan), np.zeros(n)))
        fan = n
    return layers, rng.uniform(-1, 1, fan) * np.sqrt(6.0 / fan)


def forward_row(s, row):
    """One row -> dict(yh, mag: sum of |terms| of the FM part, dmag: sum_l sum_ij |h_{l-1,i} W_l[i][j]|, z, T, hs, pres)."""
    k = s.v.shape[1]
    F = s.layers[0][0].shape[0] // k
    z = [x * s.v[i] for _, i, x in row]
    T, S = np.zeros(k), np.zeros((F, k))
    for (f, _, _), za in zip(row, z):
        T += za
        S[f] += za
    yh, mag = s.w0, abs(s.w0)
    for _, i, x in row:
        yh += s.w[i] * x
        mag += abs(s.w[i] * x)
    for a in range(len(row)):
        for b in range(a + 1, len(row)):
            t = float(z[a] @ z[b])
            yh += t
            mag += abs(t)
    hs, pres, dmag = [S.ravel()], [], 0.0
    for W, b in s.layers:
        pres.append(hs[-1] @ W + b)
        dmag += float(np.abs(hs[-1][:, None] * W).sum())
        hs.append(np.maximum(pres[-1], 0.0))
    return dict(yh=yh + float(hs[-1] @ s.u), mag=mag, dmag=dmag, z=z, T=T, hs=hs, pres=pres)


def predict(s, rows):
    """(yhat, FM magnitudes, dense magnitudes) of the rows."""
    out = [forward_row(s, r) for r in rows]
    return tuple(np.array([o[name] for o in out], np.float64) for name in ("yh", "mag", "dmag"))


def margin(s, rows):
    """The smallest |pre-activation| over the rows, the layers and the units: how far the batch is from a ReLU kink."""
    return min(float(np.abs(p).min()) for r in rows for p in forward_row(s, r)["pres"])


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


def step(s, rows, y, eta, reg0, regw, regv, regd=0.0, loss="squared", optimizer="sgd", eps=1e-10, linear=True, deep=True):
    """One mini-batch step in place -> (touched(rows), the dense gradients' sums of |per-row terms| as (layers, u))."""
    B, k = len(rows), s.v.shape[1]
    fw = [forward_row(s, r) for r in rows]
    yh, y = np.array([o["yh"] for o in fw]), np.asarray(y, np.float64)
    e = yh - y if loss == "squared" else 1.0 / (1.0 + np.exp(-yh)) - (y > 0)
    gv, gw, gu = np.zeros_like(s.v), np.zeros_like(s.w), np.zeros_like(s.u)
    gl = [(np.zeros_like(W), np.zeros_like(b)) for W, b in s.layers]
    al, au = copy.deepcopy(gl), np.zeros_like(s.u)
    for r, (row, o) in enumerate(zip(rows, fw)):
        hs, c = o["hs"], e[r] / B
        gu += c * hs[-1]
        au += np.abs(c * hs[-1])
        delta = s.u * (o["pres"][-1] > 0)
        for l in range(len(s.layers) - 1, -1, -1):
            t = c * np.outer(hs[l], delta)
            gl[l][0][:] += t
            gl[l][1][:] += c * delta
            al[l][0][:] += np.abs(t)
            al[l][1][:] += np.abs(c * delta)
            delta = s.layers[l][0] @ delta          # J when l == 0: no mask
            if l > 0:
                delta = delta * (o["pres"][l - 1] > 0)
        J = delta.reshape(-1, k)
        for (f, i, x), za in zip(row, o["z"]):
            gw[i] += c * x
            gv[i] += c * x * ((o["T"] - za) + J[f])
    g0 = e.sum() / B
    t = touched(rows, len(s.w))

    def upd(theta, n, g, mask):
        if optimizer == "sgd":
            return np.where(mask, theta - eta * g, theta), n
        n2 = n + g * g
        return np.where(mask, theta - eta * g / (np.sqrt(n2) + eps), theta), np.where(mask, n2, n)

    ada = optimizer == "adagrad"
    nv, nw, n0, nu = (s.nv, s.nw, s.n0, s.nu) if ada else (None,) * 4
    nl = s.nlayers if ada else [(None, None)] * len(s.layers)
    s.v, nv = upd(s.v, nv, gv + regv * s.v, t[:, None])
    if linear:
        s.w, nw = upd(s.w, nw, gw + regw * s.w, t)
        w0, n0 = upd(s.w0, n0, g0 + reg0 * s.w0, True)
        s.w0 = float(w0)
    if deep:
        new = [upd(W, nW, gW + regd * W, True) + upd(b, nb, gb, True) for (W, b), (nW, nb), (gW, gb) in zip(s.layers, nl, gl)]
        s.layers, nl = [(a[0], a[2]) for a in new], [(a[1], a[3]) for a in new]
        s.u, nu = upd(s.u, nu, gu + regd * s.u, True)
    if ada:
        s.nv, s.nw, s.n0, s.nu, s.nlayers = nv, nw, float(n0), nu, nl
    return t, (al, au)


def epoch(s, rows, y, batch_rows, order=None, **kw):
    n = len(rows)
    br = n if batch_rows <= 0 else batch_rows
    starts = list(range(0, n, br))
    for j in (range(len(starts)) if order is None else order):
        lo = starts[j]
        step(s, rows[lo:lo + br], y[lo:lo + br], **kw)
    return s


def planted_init(t, hidden, zero_u=False):
    """The FwFM twin's v on ffm_ref.planted(); the dense part He-uniform from the task's seed (zero_u: u = 0, the plain FM)."""
    v = np.random.default_rng(t["seed"] + 1).random((t["n1"], P_K)) / np.sqrt(P_K)
    layers, u = dense(np.random.default_rng(t["seed"] + 2), P_FIELDS, P_K, hidden)
    return State(0.0, np.zeros(t["n1"]), v, layers, u * (not zero_u), init=1.0)


def run_planted(t, hidden=(64, 32), deep=True, zero_u=False, epochs=P_EPOCHS, batch=P_BATCH):
    """Trains the twin on ffm_ref.planted() -> (state, train log-loss, test log-loss)."""
    (xtr, ytr), (xte, yte) = t["train"], t["test"]
    s = planted_init(t, hidden, zero_u)
    for _ in range(epochs):
        epoch(s, xtr, ytr, batch, eta=P_ETA, reg0=0.0, regw=0.0, regv=P_REGV, loss="logistic", optimizer="adagrad", deep=deep)
    return s, logloss(s, xtr, ytr), logloss(s, xte, yte)
