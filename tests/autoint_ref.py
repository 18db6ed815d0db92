"""The fp64 twin of AutoInt (include/fmhip_autoint.h), written as the header states it, a batch of rows at a time: the tokens by a loop
over the entries, a layer as one projection and per head two matmuls around a softmax, the chain rule a layer at a time.  Rows are lists
of (field, feature, value), as ffm_ref's; layers is a list of W_l [D_l, 4A] = [W_Q | W_K | W_V | W_R], u is [F A]."""
import numpy as np

from ffm_ref import P_BATCH, P_EPOCHS, P_ETA, P_FIELDS, P_K, P_REGV, planted, random_rows  # noqa: F401

EXP_ULP = 1.0          # the device's exp: OCML's expf, at most 1 ulp (csrc/fm_autoint.hip)
RESIDUAL_ULP = 1.2e-7 / 1e-4          # one fp32 ulp in units of the gradient tolerance TOL_G (gradients(): the residual's own terms)


class State:
    def __init__(self, w0, w, v, layers, u, heads=None, init=None):
        self.w0, self.w, self.v, self.u = float(w0), np.array(w, np.float64), np.array(v, np.float64), np.array(u, np.float64)
        self.layers = [np.array(W, np.float64) for W in layers]
        self.heads = heads          # (set by whoever knows it: the arrays do not hold it)
        if init is not None:          # AdaGrad's accumulators
            self.n0, self.nw, self.nv, self.nu = float(init), np.full_like(self.w, init), np.full_like(self.v, init), np.full_like(self.u, init)
            self.nlayers = [np.full_like(W, init) for W in self.layers]


def dense(rng, F, k, L, H, d):
    """W_l and u uniform with variance 1 / fan-in: (layers, u)."""
    A = H * d
    layers = [rng.uniform(-1, 1, (k if l == 0 else A, 4 * A)) * np.sqrt(3.0 / (k if l == 0 else A)) for l in range(L)]
    return layers, rng.uniform(-1, 1, F * A) * np.sqrt(3.0 / (F * A))


def forward(s, rows):
    """The rows -> dict(yh, mag: the linear part's sum of |terms|, cmag: the attention term's first-order forward error bound in ulps,
    keep: per layer (X, Q, K, V, [P^h], Z), xl: X_L, zmin: the smallest |pre-activation|).  The bound, E(.) elementwise: E(X_0) = sum_a
    |z_a|; a product C = A B has E(C) = E(A)|B| + |A|E(B) + |A||B|; the scores also carry |Sc - max| (the subtraction's rounding); the
    softmax's sensitivity E(P)_fg = P_fg (E(Sc)_fg + sum_g' P_fg' E(Sc)_fg') plus P_fg (EXP_ULP + log2 F + 3) for the exp, the sum's tree
    and the division — these log2 F + 3 ulps a probability are more than the chain, the sensitivity and the exp's bound alone; they are
    O(10) P beside sensitivities of O(100) and above, and TOL_Y dominates the whole — ; E(Z) = E(O) + E(R) + |Z|, the ReLU is 1-Lipschitz;
    cmag = E(X_L)|u| + |X_L||u|."""
    k, B, A = s.v.shape[1], len(rows), s.layers[0].shape[1] // 4
    F, H = len(s.u) // A, s.heads
    d = A // H
    X, EX = np.zeros((B, F, k)), np.zeros((B, F, k))
    yh, mag = np.full(B, s.w0), np.full(B, abs(s.w0))
    for r, row in enumerate(rows):
        for f, i, x in row:
            X[r, f] += x * s.v[i]
            EX[r, f] += np.abs(x * s.v[i])
            yh[r] += s.w[i] * x
            mag[r] += abs(s.w[i] * x)
    keep, zmin, csoft = [], np.inf, EXP_ULP + np.ceil(np.log2(max(F, 2))) + 3
    for W in s.layers:
        Y, EY = X @ W, EX @ np.abs(W) + np.abs(X) @ np.abs(W)
        Q, K, V, R = (Y[:, :, j * A:(j + 1) * A] for j in range(4))
        EQ, EK, EV, ER = (EY[:, :, j * A:(j + 1) * A] for j in range(4))
        O, EO, Ps = np.zeros((B, F, A)), np.zeros((B, F, A)), []
        for h in range(H):
            c = slice(h * d, (h + 1) * d)
            Sc = Q[:, :, c] @ K[:, :, c].transpose(0, 2, 1)
            Sc0 = Sc - Sc.max(axis=2, keepdims=True)
            ESc = (EQ[:, :, c] @ np.abs(K[:, :, c]).transpose(0, 2, 1) + np.abs(Q[:, :, c]) @ EK[:, :, c].transpose(0, 2, 1)
                   + np.abs(Q[:, :, c]) @ np.abs(K[:, :, c]).transpose(0, 2, 1) + np.abs(Sc0))
            P = np.exp(Sc0)
            P /= P.sum(axis=2, keepdims=True)
            EP = P * (ESc + (P * ESc).sum(axis=2, keepdims=True) + csoft)
            O[:, :, c] = P @ V[:, :, c]
            EO[:, :, c] = EP @ np.abs(V[:, :, c]) + P @ EV[:, :, c] + P @ np.abs(V[:, :, c])
            Ps.append(P)
        Z = O + R
        keep.append((X, Q, K, V, Ps, Z))
        zmin = min(zmin, np.abs(Z).min()) if Z.size else zmin
        X, EX = np.maximum(Z, 0.0), EO + ER + np.abs(Z)
    U = s.u.reshape(F, A)
    cmag = (EX * np.abs(U)).sum(axis=(1, 2)) + (np.abs(X) * np.abs(U)).sum(axis=(1, 2))
    return dict(yh=yh + (X * U).sum(axis=(1, 2)), mag=mag, cmag=cmag, keep=keep, xl=X, zmin=zmin)


def predict(s, rows):
    """(yhat, the linear part's magnitudes, the attention term's error bounds) of the rows."""
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
    """The mean loss's gradient -> dict(w0, w, v, layers [gW_l], u, absg: per dense array the sum over the rows of |terms|, as ([aW_l], au)).
    |terms| is the family's (dcn_ref, deepfm_ref): sum over the rows of |e_r| |X_l|^T |dY| on the computed values.  ONE stated addition:
    the residual is itself a difference, e = yhat - y (squared loss) or sigmoid(yhat) - t, whose operands the device knows to an fp32 ulp
    each; where they nearly agree — the step tests' one-row batch of shape (3, 4) has yhat = 0.28064584 against y = 0.28081707,
    e = -1.7e-4, at (3, 2, 32) — one ulp of the operands is 2e-4 of e, above TOL_G, and every gradient of that row inherits it.  So
    |e_r| carries one ulp of its operands, |yhat| + |y| (logistic: 1 + |yhat| / 4, sigmoid' <= 1/4), in units of TOL_G (RESIDUAL_ULP):
    at most 1.2e-3 (|yhat| + |y|) beside |e_r|, a thousandth where e is of the order of 1, and nothing that grows with the depth."""
    B, A = len(rows), s.layers[0].shape[1] // 4
    F, H = len(s.u) // A, s.heads
    d = A // H
    o = forward(s, rows)
    y = np.asarray(y, np.float64)
    e = (o["yh"] - y if loss == "squared" else 1.0 / (1.0 + np.exp(-o["yh"])) - (y > 0)) / B
    ae = np.abs(e) + RESIDUAL_ULP * (np.abs(o["yh"]) + np.abs(y) if loss == "squared" else 1.0 + np.abs(o["yh"]) / 4) / B
    G = np.tile(s.u.reshape(1, F, A), (B, 1, 1))
    gW, aW = [], []
    for l in range(len(s.layers) - 1, -1, -1):
        X, Q, K, V, Ps, Z = o["keep"][l]
        Gz = G * (Z > 0)
        dY = np.zeros((B, F, 4 * A))
        dY[:, :, 3 * A:] = Gz
        for h in range(H):
            c, P = slice(h * d, (h + 1) * d), Ps[h]
            dP = Gz[:, :, c] @ V[:, :, c].transpose(0, 2, 1)
            dSc = P * (dP - (dP * P).sum(axis=2, keepdims=True))
            dY[:, :, h * d:(h + 1) * d] = dSc @ K[:, :, c]
            dY[:, :, A + h * d:A + (h + 1) * d] = dSc.transpose(0, 2, 1) @ Q[:, :, c]
            dY[:, :, 2 * A + h * d:2 * A + (h + 1) * d] = P.transpose(0, 2, 1) @ Gz[:, :, c]
        gW.insert(0, np.einsum("b,bfd,bfn->dn", e, X, dY))
        aW.insert(0, np.einsum("b,bfd,bfn->dn", ae, np.abs(X), np.abs(dY)))
        G = dY @ s.layers[l].T
    gv, gw = np.zeros_like(s.v), np.zeros_like(s.w)
    for r, row in enumerate(rows):
        for f, i, x in row:
            gw[i] += e[r] * x
            gv[i] += e[r] * x * G[r, f]
    xl = o["xl"].reshape(B, F * A)
    return dict(w0=e.sum(), w=gw, v=gv, layers=gW, u=e @ xl, absg=(aW, ae @ np.abs(xl)))


def step(s, rows, y, eta, reg0, regw, regv, regd=0.0, loss="squared", optimizer="sgd", eps=1e-10, linear=True, attention=True):
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
    if attention:
        new = [upd(W, n, g + regd * W, True) for W, n, g in zip(s.layers, nl, G["layers"])]
        s.layers, nl = [a for a, _ in new], [b for _, b in new]
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


def planted_init(t, L=2, H=2, d=16):
    """The FwFM twin's v on ffm_ref.planted(); the attention part at its init scale from the task's seed."""
    v = np.random.default_rng(t["seed"] + 1).random((t["n1"], P_K)) / np.sqrt(P_K)
    layers, u = dense(np.random.default_rng(t["seed"] + 2), P_FIELDS, P_K, L, H, d)
    return State(0.0, np.zeros(t["n1"]), v, layers, u, heads=H, init=1.0)


def run_planted(t, L=2, H=2, d=16, epochs=P_EPOCHS, batch=P_BATCH):
    """Trains the twin on ffm_ref.planted() -> (state, train log-loss, test log-loss)."""
    (xtr, ytr), (xte, yte) = t["train"], t["test"]
    s = planted_init(t, L, H, d)
    for _ in range(epochs):
        epoch(s, xtr, ytr, batch, eta=P_ETA, reg0=0.0, regw=0.0, regv=P_REGV, loss="logistic", optimizer="adagrad")
    return s, logloss(s, xtr, ytr), logloss(s, xte, yte)
