"""The fp64 twin of the PNN (include/fmhip_pnn.h), written as the header states it: the pairs as a double loop over i < j, the MLP as
one matmul a layer, the chain rule a layer at a time.  Rows are lists of (field, feature, value), as ffm_ref's; layers is a list of
(W_l [n_{l-1}, n_l], b_l [n_l]) with n_0 = F k + F (F - 1) / 2, u is [n_L]."""
import copy

import numpy as np

from deepfm_ref import State, touched  # noqa: F401
from ffm_ref import P_BATCH, P_EPOCHS, P_ETA, P_FIELDS, P_K, P_REGV, planted, random_rows  # noqa: F401


def width(F, k):
    return F * k + F * (F - 1) // 2


def fields(s):
    """F, from W_1's height and k."""
    k, n0 = s.v.shape[1], s.layers[0][0].shape[0]
    return next(F for F in range(1, 65) if width(F, k) == n0)


def dense(rng, F, k, hidden):
    """He-uniform layers and u, zero biases: (layers, u)."""
    layers, fan = [], width(F, k)
    for n in hidden:
        layers.append((rng.uniform(-1, 1, (fan, n)) * np.sqrt(6.0 / fan), np.zeros(n)))
        fan = n
    return layers, rng.uniform(-1, 1, fan) * np.sqrt(6.0 / fan)


def forward_row(s, row):
    """One row -> dict(yh, mag: sum of |terms| of the linear part, dmag: the dense products' sum of |terms| — a pair row of W_1 under
    sum_d |S_id S_jd|, the chain's own terms: g_p can cancel —, S, habs: h_0 with those sums in the pairs' places, hs, pres)."""
    k, F = s.v.shape[1], fields(s)
    S = np.zeros((F, k))
    yh, mag = s.w0, abs(s.w0)
    for f, i, x in row:
        S[f] += x * s.v[i]
        yh += s.w[i] * x
        mag += abs(s.w[i] * x)
    g, gabs = [], []
    for i in range(F):
        for j in range(i + 1, F):
            g.append(float(S[i] @ S[j]))
            gabs.append(float(np.abs(S[i] * S[j]).sum()))
    hs, pres = [np.concatenate([S.ravel(), g])], []
    habs = np.concatenate([np.abs(S.ravel()), gabs])
    dmag = 0.0
    for l, (W, b) in enumerate(s.layers):
        pres.append(hs[-1] @ W + b)
        dmag += float(((habs if l == 0 else np.abs(hs[-1]))[:, None] * np.abs(W)).sum())
        hs.append(np.maximum(pres[-1], 0.0))
    return dict(yh=yh + float(hs[-1] @ s.u), mag=mag, dmag=dmag, S=S, habs=habs, hs=hs, pres=pres)


def predict(s, rows):
    """(yhat, the linear part's magnitudes, the dense magnitudes) of the rows."""
    out = [forward_row(s, r) for r in rows]
    return tuple(np.array([o[name] for o in out], np.float64) for name in ("yh", "mag", "dmag"))


def margin(s, rows):
    """The smallest |pre-activation| over the rows, the layers and the units: how far the batch is from a ReLU kink."""
    return min(float(np.abs(p).min()) for r in rows for p in forward_row(s, r)["pres"])


def logloss(s, rows, y):
    yh = predict(s, rows)[0]
    return float(np.mean(np.maximum(yh, 0.0) - (y > 0) * yh + np.log1p(np.exp(-np.abs(yh)))))


def gradients(s, rows, y, loss="squared"):
    """The mean loss's gradient -> dict(w0, w, v, layers [(gW, gb)], u, and al, au: the dense gradients' sums of |per-row terms|)."""
    B, k, F = len(rows), s.v.shape[1], fields(s)
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
            gl[l][0][:] += c * np.outer(hs[l], delta)
            gl[l][1][:] += c * delta
            al[l][0][:] += np.abs(c * np.outer(o["habs"] if l == 0 else hs[l], delta))
            al[l][1][:] += np.abs(c * delta)
            delta = s.layers[l][0] @ delta          # [Js | dg] when l == 0: no mask
            if l > 0:
                delta = delta * (o["pres"][l - 1] > 0)
        J, dg, p = delta[:F * k].reshape(F, k).copy(), delta[F * k:], 0
        for i in range(F):
            for j in range(i + 1, F):
                J[i] += dg[p] * o["S"][j]
                J[j] += dg[p] * o["S"][i]
                p += 1
        for f, i, x in row:
            gw[i] += c * x
            gv[i] += c * x * J[f]
    return dict(w0=e.sum() / B, w=gw, v=gv, layers=gl, u=gu, al=al, au=au)


def step(s, rows, y, eta, reg0, regw, regv, regd=0.0, loss="squared", optimizer="sgd", eps=1e-10, linear=True, deep=True):
    """One mini-batch step in place -> (touched(rows), the dense gradients' sums of |per-row terms| as (layers, u))."""
    G = gradients(s, rows, y, loss)
    t = touched(rows, len(s.w))

    def upd(theta, n, g, mask):
        if optimizer == "sgd":
            return np.where(mask, theta - eta * g, theta), n
        n2 = n + g * g
        return np.where(mask, theta - eta * g / (np.sqrt(n2) + eps), theta), np.where(mask, n2, n)

    ada = optimizer == "adagrad"
    nv, nw, n0, nu = (s.nv, s.nw, s.n0, s.nu) if ada else (None,) * 4
    nl = s.nlayers if ada else [(None, None)] * len(s.layers)
    s.v, nv = upd(s.v, nv, G["v"] + regv * s.v, t[:, None])
    if linear:
        s.w, nw = upd(s.w, nw, G["w"] + regw * s.w, t)
        w0, n0 = upd(s.w0, n0, G["w0"] + reg0 * s.w0, True)
        s.w0 = float(w0)
    if deep:
        new = [upd(W, nW, gW + regd * W, True) + upd(b, nb, gb, True) for (W, b), (nW, nb), (gW, gb) in zip(s.layers, nl, G["layers"])]
        s.layers, nl = [(a[0], a[2]) for a in new], [(a[1], a[3]) for a in new]
        s.u, nu = upd(s.u, nu, G["u"] + regd * s.u, True)
    if ada:
        s.nv, s.nw, s.n0, s.nu, s.nlayers = nv, nw, float(n0), nu, nl
    return t, (G["al"], G["au"])


def planted_init(t, hidden):
    """The FwFM twin's v on ffm_ref.planted(); the dense part He-uniform from the task's seed."""
    v = np.random.default_rng(t["seed"] + 1).random((t["n1"], P_K)) / np.sqrt(P_K)
    layers, u = dense(np.random.default_rng(t["seed"] + 2), P_FIELDS, P_K, hidden)
    return State(0.0, np.zeros(t["n1"]), v, layers, u, init=1.0)


def run_planted(t, hidden=(64, 32), epochs=P_EPOCHS, batch=P_BATCH):
    """Trains the twin on ffm_ref.planted() -> (state, train log-loss, test log-loss)."""
    (xtr, ytr), (xte, yte) = t["train"], t["test"]
    s = planted_init(t, hidden)
    for _ in range(epochs):
        for lo in range(0, len(xtr), batch):
            step(s, xtr[lo:lo + batch], ytr[lo:lo + batch], eta=P_ETA, reg0=0.0, regw=0.0, regv=P_REGV, loss="logistic", optimizer="adagrad")
    return s, logloss(s, xtr, ytr), logloss(s, xte, yte)
