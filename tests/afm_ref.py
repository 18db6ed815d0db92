"""The fp64 twin of the Attentional Factorization Machine (include/fmhip_afm.h), written as the header states it, a row at a time, every
pair (i < j) explicitly.  Rows are lists of (field, feature, value), as ffm_ref's.  A unit (row, pair, hidden unit) is NEAR THE KINK when
|W E + b| < KINK x its own sum of |terms|: an fp32 run may take its ReLU mask either way.  Such a unit's full absolute contribution is
added to every bound it feeds — once more into delta_ij, and as if its mask were on into the dense arrays' sums of |terms|."""
import numpy as np

from cin_ref import touched  # noqa: F401
from ffm_ref import P_BATCH, P_EPOCHS, P_ETA, P_FIELDS, P_K, P_REGV, planted, random_rows  # noqa: F401

KINK = 4 * 1.2e-7
DENSE = ("W", "b", "h", "p")


class State:
    def __init__(self, w0, w, v, W, b, h, p, init=None):
        self.w0 = float(w0)
        self.w, self.v, self.W, self.b, self.h, self.p = (np.array(x, np.float64) for x in (w, v, W, b, h, p))
        if init is not None:          # AdaGrad's accumulators
            self.n0 = float(init)
            for name in ("w", "v") + DENSE:
                setattr(self, "n" + name, np.full_like(getattr(self, name), init))

    # the dense part as cin_ref.State names it, so that test_gpu_cin.check_dense serves: layers + [u] = W, b, h, p
    layers, u = property(lambda s: [s.W, s.b, s.h]), property(lambda s: s.p)
    nlayers, nu = property(lambda s: [s.nW, s.nb, s.nh]), property(lambda s: s.np)


def dense(rng, k, t, gain=1.0):
    """(W, b, h, p): W, h and p uniform with variance gain^2 / fan-in (fan-in k, t, k), b ~ N(0, (gain / 4)^2)."""
    u = lambda shape, fan: rng.uniform(-1, 1, shape) * gain * np.sqrt(3.0 / fan)
    return u((t, k), k), rng.normal(0, 0.25 * gain, t), u(t, t), u(k, k)


def _row(s, row, F):
    """One row -> dict(lin, mag, S, and — with F >= 2 — iu, ju, E, pre, near, H, a, c, o, T, bound)."""
    S, lin, mag = np.zeros((F, s.v.shape[1])), s.w0, abs(s.w0)
    for f, i, x in row:
        S[f] += x * s.v[i]
        lin += s.w[i] * x
        mag += abs(s.w[i] * x)
    r = dict(lin=lin, mag=mag, S=S, T=0.0, bound=0.0, units=0, near_n=0)
    if F < 2:
        return r
    iu, ju = np.triu_indices(F, 1)
    E = S[iu] * S[ju]
    pre, sab = E @ s.W.T + s.b, np.abs(E) @ np.abs(s.W).T + np.abs(s.b)
    near = np.abs(pre) < KINK * sab
    H = np.maximum(pre, 0.0)
    sc = H @ s.h
    a = np.exp(sc - sc.max())
    a /= a.sum()
    c, o = E @ s.p, a @ E
    T = a @ c
    delta = (sab * (1 + near)) @ np.abs(s.h)
    r.update(iu=iu, ju=ju, E=E, pre=pre, near=near, H=H, a=a, c=c, o=o, T=T, smax=sc.max(), units=near.size, near_n=int(near.sum()),
             bound=a @ (np.abs(c - T) * delta) + a @ (np.abs(E) @ np.abs(s.p)))
    return r


def predict(s, rows, F, full=False):
    """(yhat, the linear part's magnitudes, the AFM term's first-order forward bounds at unit rounding[, the largest scores])."""
    out = [_row(s, row, F) for row in rows]
    res = tuple(np.array([r[key] for r in out]) for key in ("lin", "mag", "bound"))
    res = (res[0] + np.array([r["T"] for r in out]),) + res[1:]
    return res + (np.array([r.get("smax", 0.0) for r in out]),) if full else res


def logloss(s, rows, y, F):
    yh = predict(s, rows, F)[0]
    return float(np.mean(np.maximum(yh, 0.0) - (y > 0) * yh + np.log1p(np.exp(-np.abs(yh)))))


def gradients(s, rows, y, F, loss="squared"):
    """The mean loss's gradient -> dict(w0, w, v, W, b, h, p, absg: DENSE's sums over the rows of |terms|, share: of units near the
    kink, margin: the smallest |pre-activation|)."""
    B, y = len(rows), np.asarray(y, np.float64)
    G = {name: np.zeros_like(getattr(s, name)) for name in ("w", "v") + DENSE}
    A = {name: np.zeros_like(getattr(s, name)) for name in DENSE}
    g0, units, near_n, margin = 0.0, 0, 0, np.inf
    for row, yr in zip(rows, y):
        r = _row(s, row, F)
        yh = r["lin"] + r["T"]
        e = (yh - yr if loss == "squared" else 1.0 / (1.0 + np.exp(-yh)) - (yr > 0)) / B
        g0 += e
        J = np.zeros_like(r["S"])
        if F >= 2:
            E, a, S, iu, ju = r["E"], r["a"], r["S"], r["iu"], r["ju"]
            ds, mask = a * (r["c"] - r["T"]), r["pre"] > 0
            dH, adH = ds[:, None] * s.h * mask, np.abs(ds)[:, None] * np.abs(s.h) * (mask | r["near"])
            for name, g, ab in (("h", ds @ r["H"], np.abs(ds) @ r["H"]), ("b", dH.sum(0), adH.sum(0)), ("W", dH.T @ E, adH.T @ np.abs(E)),
                                ("p", r["o"], a @ np.abs(E))):
                G[name] += e * g
                A[name] += abs(e) * ab
            dE = a[:, None] * s.p + dH @ s.W
            np.add.at(J, iu, dE * S[ju])
            np.add.at(J, ju, dE * S[iu])
            units, near_n, margin = units + r["units"], near_n + r["near_n"], min(margin, np.abs(r["pre"]).min())
        for f, i, x in row:
            G["w"][i] += e * x
            G["v"][i] += e * x * J[f]
    return dict(G, w0=g0, absg=([A["W"], A["b"], A["h"]], A["p"]), share=near_n / max(units, 1), margin=margin)


def step(s, rows, y, F, eta, reg0, regw, regv, regd=0.0, loss="squared", optimizer="sgd", eps=1e-10, linear=True, attention=True):
    """One mini-batch step in place -> (touched(rows), the dense gradients' sums of |per-row terms|, the share of units near the kink)."""
    G, t, ada = gradients(s, rows, y, F, loss), touched(rows, len(s.w)), optimizer == "adagrad"

    def upd(name, reg, mask):
        theta, g = getattr(s, name), G[name] + reg * getattr(s, name)
        if not ada:
            new = np.where(mask, theta - eta * g, theta)
        else:
            acc = "n0" if name == "w0" else "n" + name
            n = getattr(s, acc)
            n2 = n + g * g
            new = np.where(mask, theta - eta * g / (np.sqrt(n2) + eps), theta)
            setattr(s, acc, np.where(mask, n2, n) if np.ndim(n2) else float(n2))
        setattr(s, name, new if np.ndim(new) else float(new))

    upd("v", regv, t[:, None])
    if linear:
        upd("w", regw, t)
        upd("w0", reg0, True)
    if attention:
        for name in DENSE:
            upd(name, regd, True)
    return t, G["absg"], G["share"]


def planted_init(t, attention=16):
    """The FwFM twin's v on ffm_ref.planted(); the attention part at its init scale from the task's seed."""
    v = np.random.default_rng(t["seed"] + 1).random((t["n1"], P_K)) / np.sqrt(P_K)
    return State(0.0, np.zeros(t["n1"]), v, *dense(np.random.default_rng(t["seed"] + 2), P_K, attention), init=1.0)


def run_planted(t, attention=16, epochs=P_EPOCHS, batch=P_BATCH):
    """Trains the twin on ffm_ref.planted() -> (state, train log-loss, test log-loss)."""
    (xtr, ytr), (xte, yte) = t["train"], t["test"]
    s = planted_init(t, attention)
    for lo in list(range(0, len(xtr), batch)) * epochs:
        step(s, xtr[lo:lo + batch], ytr[lo:lo + batch], P_FIELDS, P_ETA, 0.0, 0.0, P_REGV, loss="logistic", optimizer="adagrad")
    return s, logloss(s, xtr, ytr, P_FIELDS), logloss(s, xte, yte, P_FIELDS)
