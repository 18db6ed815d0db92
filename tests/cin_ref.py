"""The fp64 twin of the Compressed Interaction Network (include/fmhip_cin.h), written as the header states it, a chunk of rows at a
time: the field sums by a loop over the entries, a layer as the explicit Khatri-Rao operand Z[(row, d), (i, j)] = X^{l-1}[i, d] X^0[j, d]
times W_l, the chain rule a layer at a time.  Rows are lists of (field, feature, value), as ffm_ref's; layers is a list of
W_l [H_l, H_{l-1}, F], u is [H_1 + .. + H_L]."""
import numpy as np

from ffm_ref import P_BATCH, P_EPOCHS, P_ETA, P_FIELDS, P_K, P_REGV, planted, random_rows  # noqa: F401

CHUNK = 64          # rows whose Z is held at a time


class State:
    def __init__(self, w0, w, v, layers, u, init=None):
        self.w0, self.w, self.v, self.u = float(w0), np.array(w, np.float64), np.array(v, np.float64), np.array(u, np.float64)
        self.layers = [np.array(W, np.float64) for W in layers]
        if init is not None:          # AdaGrad's accumulators
            self.n0, self.nw, self.nv, self.nu = float(init), np.full_like(self.w, init), np.full_like(self.v, init), np.full_like(self.u, init)
            self.nlayers = [np.full_like(W, init) for W in self.layers]


def dense(rng, F, k, maps, gain=1.0):
    """W_l and u uniform with variance gain^2 / fan-in (fan-in H_{l-1} F, sum H_l): (layers, u)."""
    layers, prev = [], F
    for h in maps:
        layers.append(rng.uniform(-1, 1, (h, prev, F)) * gain * np.sqrt(3.0 / (prev * F)))
        prev = h
    return layers, rng.uniform(-1, 1, sum(maps)) * np.sqrt(3.0 / sum(maps))


def _chunk(s, rows):
    """One chunk -> dict(yh, mag, cmag, xs: X^0 .. X^L [B, H_l, k], zs: Z_l [B k, H_{l-1} F], ps: [B, sum H]).  The bound, layer by
    layer at unit rounding: E(X^0) = sum_a |z_a| per slot; a term W Xp X0 carries E(Xp)|X0| + |Xp| E(X0) and two units of its own
    magnitude (the product sum's and the A operand's pre-multiply); E(p) = sum_d (E(X) + |X|); cmag = sum_l (E(p^l) + |p^l|) |u^l|."""
    k, F, B = s.v.shape[1], s.layers[0].shape[2], len(rows)
    x0, e0 = np.zeros((B, F, k)), np.zeros((B, F, k))
    yh, mag = np.full(B, s.w0), np.full(B, abs(s.w0))
    for r, row in enumerate(rows):
        for f, i, x in row:
            x0[r, f] += x * s.v[i]
            e0[r, f] += np.abs(x * s.v[i])
            yh[r] += s.w[i] * x
            mag[r] += abs(s.w[i] * x)
    kr = lambda a, b: (a.transpose(0, 2, 1)[:, :, :, None] * b.transpose(0, 2, 1)[:, :, None, :]).reshape(B * k, -1)          # [B k, (i, j)]
    xs, zs, ps, ex, eps_ = [x0], [], [], e0, []
    for W in s.layers:
        Wf, xp = W.reshape(W.shape[0], -1), xs[-1]
        z = kr(xp, x0)
        ez = kr(ex, np.abs(x0)) + kr(np.abs(xp), e0) + 2 * np.abs(z)
        x = (z @ Wf.T).reshape(B, k, -1).transpose(0, 2, 1)
        ex = (ez @ np.abs(Wf).T).reshape(B, k, -1).transpose(0, 2, 1)
        zs.append(z)
        xs.append(x)
        ps.append(x.sum(2))
        eps_.append((ex + np.abs(x)).sum(2))
    p, ep = np.concatenate(ps, 1), np.concatenate(eps_, 1)
    return dict(yh=yh + p @ s.u, mag=mag, cmag=(ep + np.abs(p)) @ np.abs(s.u), xs=xs, zs=zs, ps=p)


def forward(s, rows):
    """The rows -> dict(yh, mag: the linear part's sum of |terms|, cmag: the CIN term's first-order forward error bound at unit
    rounding, rms: the rms of X^1 .. X^L over the rows), CHUNK rows at a time."""
    outs = [_chunk(s, rows[lo:lo + CHUNK]) for lo in range(0, len(rows), CHUNK)]
    sq = [sum((o["xs"][l] ** 2).sum() for o in outs) / sum(o["xs"][l].size for o in outs) for l in range(1, len(s.layers) + 1)]
    return dict(yh=np.concatenate([o["yh"] for o in outs]), mag=np.concatenate([o["mag"] for o in outs]),
                cmag=np.concatenate([o["cmag"] for o in outs]), rms=np.sqrt(sq))


def predict(s, rows):
    """(yhat, the linear part's magnitudes, the CIN term's error bounds) of the rows."""
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
    """The mean loss's gradient -> dict(w0, w, v, layers [gW_l], u, absg: per dense array the sum over the rows of |terms|, as
    ([aW_l], au))."""
    B, k, L = len(rows), s.v.shape[1], len(s.layers)
    y = np.asarray(y, np.float64)
    maps = [W.shape[0] for W in s.layers]
    uo = np.concatenate([[0], np.cumsum(maps)])
    gW, aW = [np.zeros_like(W) for W in s.layers], [np.zeros_like(W) for W in s.layers]
    gu, au, gv, gw, g0 = np.zeros_like(s.u), np.zeros_like(s.u), np.zeros_like(s.v), np.zeros_like(s.w), 0.0
    for lo in range(0, B, CHUNK):
        part = rows[lo:lo + CHUNK]
        o, b = _chunk(s, part), len(part)
        e = (o["yh"] - y[lo:lo + b] if loss == "squared" else 1.0 / (1.0 + np.exp(-o["yh"])) - (y[lo:lo + b] > 0)) / B
        x0, em = o["xs"][0], np.repeat(e, k)[:, None]          # em: the residual of an M-row (row, d)
        g0 += e.sum()
        gu += e @ o["ps"]
        au += np.abs(e[:, None] * o["ps"]).sum(0)
        G = np.tile(s.u[uo[L - 1]:uo[L]][None, :, None], (b, 1, k))          # G^L [b, H_L, k]
        J = np.zeros_like(x0)
        for l in range(L, 0, -1):
            W, xp = s.layers[l - 1], o["xs"][l - 1]
            Gm = G.transpose(0, 2, 1).reshape(b * k, -1)          # [b k, H_l]
            gW[l - 1] += ((em * Gm).T @ o["zs"][l - 1]).reshape(W.shape)
            aW[l - 1] += (np.abs(em * Gm).T @ np.abs(o["zs"][l - 1])).reshape(W.shape)
            dZ = (Gm @ W.reshape(W.shape[0], -1)).reshape(b, k, W.shape[1], W.shape[2])          # [b, d, i, j]
            J += np.einsum("bdij,bid->bjd", dZ, xp)
            G = np.einsum("bdij,bjd->bid", dZ, x0)
            if l >= 2:
                G = G + s.u[uo[l - 2]:uo[l - 1]][None, :, None]
        J += G
        for r, row in enumerate(part):
            for f, i, x in row:
                gw[i] += e[r] * x
                gv[i] += e[r] * x * J[r, f]
    return dict(w0=g0, w=gw, v=gv, layers=gW, u=gu, absg=(aW, au))


def step(s, rows, y, eta, reg0, regw, regv, regd=0.0, loss="squared", optimizer="sgd", eps=1e-10, linear=True, cin=True):
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
    nl = s.nlayers if ada else [None] * len(s.layers)
    s.v, nv = upd(s.v, nv, G["v"] + regv * s.v, t[:, None])
    if linear:
        s.w, nw = upd(s.w, nw, G["w"] + regw * s.w, t)
        w0, n0 = upd(s.w0, n0, G["w0"] + reg0 * s.w0, True)
        s.w0 = float(w0)
    if cin:
        new = [upd(W, n, g + regd * W, True) for W, n, g in zip(s.layers, nl, G["layers"])]
        s.layers, nl = [a[0] for a in new], [a[1] for a in new]
        s.u, nu = upd(s.u, nu, G["u"] + regd * s.u, True)
    if ada:
        s.nv, s.nw, s.n0, s.nu, s.nlayers = nv, nw, float(n0), nu, nl
    return t, G["absg"]


def epoch(s, rows, y, batch_rows, order=None, **kw):
    n = len(rows)
    br = n if batch_rows <= 0 else batch_rows
    starts = list(range(0, n, br))
    for j in (range(len(starts)) if order is None else order):
        lo = starts[j]
        step(s, rows[lo:lo + br], y[lo:lo + br], **kw)
    return s


def planted_init(t, maps=(16, 16)):
    """The FwFM twin's v on ffm_ref.planted(); the CIN part at its init scale from the task's seed."""
    v = np.random.default_rng(t["seed"] + 1).random((t["n1"], P_K)) / np.sqrt(P_K)
    layers, u = dense(np.random.default_rng(t["seed"] + 2), P_FIELDS, P_K, maps)
    return State(0.0, np.zeros(t["n1"]), v, layers, u, init=1.0)


def run_planted(t, maps=(16, 16), epochs=P_EPOCHS, batch=P_BATCH):
    """Trains the twin on ffm_ref.planted() -> (state, train log-loss, test log-loss)."""
    (xtr, ytr), (xte, yte) = t["train"], t["test"]
    s = planted_init(t, maps)
    for _ in range(epochs):
        epoch(s, xtr, ytr, batch, eta=P_ETA, reg0=0.0, regw=0.0, regv=P_REGV, loss="logistic", optimizer="adagrad")
    return s, logloss(s, xtr, ytr), logloss(s, xte, yte)
