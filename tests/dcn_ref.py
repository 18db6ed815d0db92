"""The fp64 twin of the low-rank cross network (include/fmhip_dcn.h), written as the header states it, a batch of rows at a time: the
field sums by a loop over the entries, a layer as two matmuls, the chain rule a layer at a time.  Rows are lists of (field, feature,
value), as ffm_ref's; cross is a list of (V_l [F k, r], U_l [r, F k], c_l [F k]), u is [F k]."""
import numpy as np

from ffm_ref import P_BATCH, P_EPOCHS, P_ETA, P_FIELDS, P_K, P_REGV, planted, random_rows  # noqa: F401


class State:
    def __init__(self, w0, w, v, cross, u, init=None):
        self.w0, self.w, self.v, self.u = float(w0), np.array(w, np.float64), np.array(v, np.float64), np.array(u, np.float64)
        self.cross = [tuple(np.array(x, np.float64) for x in t) for t in cross]
        if init is not None:          # AdaGrad's accumulators
            self.n0, self.nw, self.nv, self.nu = float(init), np.full_like(self.w, init), np.full_like(self.v, init), np.full_like(self.u, init)
            self.ncross = [tuple(np.full_like(x, init) for x in t) for t in self.cross]


def dense(rng, F, k, layers, rank, c_std=0.0):
    """V_l, U_l and u uniform with variance 1 / fan-in, c_l ~ N(0, c_std^2): (cross, u)."""
    P = F * k
    cross = [(rng.uniform(-1, 1, (P, rank)) * np.sqrt(3.0 / P), rng.uniform(-1, 1, (rank, P)) * np.sqrt(3.0 / rank), rng.normal(0, 1, P) * c_std)
             for _ in range(layers)]
    return cross, rng.uniform(-1, 1, P) * np.sqrt(3.0 / P)


def forward(s, rows):
    """The rows -> dict(yh, mag: the linear part's sum of |terms|, cmag: the cross term's first-order forward error bound at unit
    rounding, xs: x_0 .. x_L [B, P], ts, ps).  The bound, layer by layer: E(x_0) = sum_a |z_a| per slot, E(t) = E(x)|V| + |x||V|,
    E(p) = E(t)|U| + |t||U| + |c|, E(x_{l+1}) = |x_0| E(p) + |p| E(x_0) + E(x_l) + |x_0||p| + |x_l|, cmag = E(x_L)|u| + |x_L||u|."""
    k, B = s.v.shape[1], len(rows)
    x0, e0 = np.zeros((B, len(s.u))), np.zeros((B, len(s.u)))
    yh, mag = np.full(B, s.w0), np.full(B, abs(s.w0))
    for r, row in enumerate(rows):
        for f, i, x in row:
            x0[r, f * k:(f + 1) * k] += x * s.v[i]
            e0[r, f * k:(f + 1) * k] += np.abs(x * s.v[i])
            yh[r] += s.w[i] * x
            mag[r] += abs(s.w[i] * x)
    xs, ts, ps, ex = [x0], [], [], e0
    for V, U, c in s.cross:
        x = xs[-1]
        t = x @ V
        p = t @ U + c
        et = ex @ np.abs(V) + np.abs(x) @ np.abs(V)
        ep = et @ np.abs(U) + np.abs(t) @ np.abs(U) + np.abs(c)
        ex = np.abs(x0) * ep + np.abs(p) * e0 + ex + np.abs(x0 * p) + np.abs(x)
        ts.append(t)
        ps.append(p)
        xs.append(x0 * p + x)
    cmag = ex @ np.abs(s.u) + np.abs(xs[-1]) @ np.abs(s.u)
    return dict(yh=yh + xs[-1] @ s.u, mag=mag, cmag=cmag, xs=xs, ts=ts, ps=ps)


def predict(s, rows):
    """(yhat, the linear part's magnitudes, the cross term's error bounds) of the rows."""
    o = forward(s, rows)
    return o["yh"], o["mag"], o["cmag"]


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


def gradients(s, rows, y, loss="squared"):
    """The mean loss's gradient -> dict(w0, w, v, cross [(gV, gU, gc)], u, absg: per dense array the sum over the rows of |terms|, as
    ([(aV, aU, ac)], au))."""
    B, k = len(rows), s.v.shape[1]
    o = forward(s, rows)
    y = np.asarray(y, np.float64)
    e = (o["yh"] - y if loss == "squared" else 1.0 / (1.0 + np.exp(-o["yh"])) - (y > 0)) / B
    xs, x0, ec = o["xs"], o["xs"][0], e[:, None]
    g = np.tile(s.u, (B, 1))          # g_L
    J2, gc, ac = np.zeros_like(x0), [], []
    for l in range(len(s.cross) - 1, -1, -1):
        V, U, _ = s.cross[l]
        q = g * x0
        m = q @ U.T
        J2 += g * o["ps"][l]
        gc.insert(0, ((ec * xs[l]).T @ m, (ec * o["ts"][l]).T @ q, (ec * q).sum(0)))
        ac.insert(0, (np.abs(ec * xs[l]).T @ np.abs(m), np.abs(ec * o["ts"][l]).T @ np.abs(q), np.abs(ec * q).sum(0)))
        g = m @ V.T + g
    J = g + J2
    gv, gw = np.zeros_like(s.v), np.zeros_like(s.w)
    for r, row in enumerate(rows):
        for f, i, x in row:
            gw[i] += e[r] * x
            gv[i] += e[r] * x * J[r, f * k:(f + 1) * k]
    return dict(w0=e.sum(), w=gw, v=gv, cross=gc, u=(ec * xs[-1]).sum(0), absg=(ac, np.abs(ec * xs[-1]).sum(0)))


def step(s, rows, y, eta, reg0, regw, regv, regd=0.0, loss="squared", optimizer="sgd", eps=1e-10, linear=True, cross=True):
    """One mini-batch step in place -> (touched(rows), the dense gradients' sums of |per-row terms|)."""
    G = gradients(s, rows, y, loss)
    t = touched(rows, len(s.w))

    def upd(theta, n, g, mask):
        if optimizer == "sgd":
            return np.where(mask, theta - eta * g, theta), n
        n2 = n + g * g
        return np.where(mask, theta - eta * g / (np.sqrt(n2) + eps), theta), np.where(mask, n2, n)

    ada = optimizer == "adagrad"
    nv, nw, n0, nu = (s.nv, s.nw, s.n0, s.nu) if ada else (None,) * 4
    nc = s.ncross if ada else [(None,) * 3] * len(s.cross)
    s.v, nv = upd(s.v, nv, G["v"] + regv * s.v, t[:, None])
    if linear:
        s.w, nw = upd(s.w, nw, G["w"] + regw * s.w, t)
        w0, n0 = upd(s.w0, n0, G["w0"] + reg0 * s.w0, True)
        s.w0 = float(w0)
    if cross:
        new = [[upd(th, n, g + reg * th, True) for th, n, g, reg in zip(T, N, Gl, (regd, regd, 0.0))] for T, N, Gl in zip(s.cross, nc, G["cross"])]
        s.cross, nc = [tuple(a[0] for a in layer) for layer in new], [tuple(a[1] for a in layer) for layer in new]
        s.u, nu = upd(s.u, nu, G["u"] + regd * s.u, True)
    if ada:
        s.nv, s.nw, s.n0, s.nu, s.ncross = nv, nw, float(n0), nu, nc
    return t, G["absg"]


def epoch(s, rows, y, batch_rows, order=None, **kw):
    n = len(rows)
    br = n if batch_rows <= 0 else batch_rows
    starts = list(range(0, n, br))
    for j in (range(len(starts)) if order is None else order):
        lo = starts[j]
        step(s, rows[lo:lo + br], y[lo:lo + br], **kw)
    return s


def planted_init(t, layers=2, rank=16):
    """The FwFM twin's v on ffm_ref.planted(); the cross part at its init scale from the task's seed."""
    v = np.random.default_rng(t["seed"] + 1).random((t["n1"], P_K)) / np.sqrt(P_K)
    cross, u = dense(np.random.default_rng(t["seed"] + 2), P_FIELDS, P_K, layers, rank)
    return State(0.0, np.zeros(t["n1"]), v, cross, u, init=1.0)


def run_planted(t, layers=2, rank=16, epochs=P_EPOCHS, batch=P_BATCH):
    """Trains the twin on ffm_ref.planted() -> (state, train log-loss, test log-loss)."""
    (xtr, ytr), (xte, yte) = t["train"], t["test"]
    s = planted_init(t, layers, rank)
    for _ in range(epochs):
        epoch(s, xtr, ytr, batch, eta=P_ETA, reg0=0.0, regw=0.0, regv=P_REGV, loss="logistic", optimizer="adagrad")
    return s, logloss(s, xtr, ytr), logloss(s, xte, yte)
