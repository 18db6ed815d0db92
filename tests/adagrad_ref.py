"""fp64 reference of the AdaGrad update (fmhip_model_set_optimizer, FMHIP_OPT_ADAGRAD) for the tests.

The gradient is the oracle's (oracle.batch_grad, fp64); the logistic loss goes through the pseudo-target trick of
test_gpu_logistic.py (the squared residual at y' = yhat - (sigmoid(yhat) - t) is the logistic one).  The rule, per scalar
parameter theta with its accumulator n (torch.optim.Adagrad with lr = eta, weight_decay = reg, lr_decay = 0):
    g_hat = g/|B| + reg*theta,   n <- n + g_hat^2,   theta <- theta - eta*g_hat / (sqrt(n) + eps)
test_host_adagrad.py pins `adagrad_rule` to torch.optim.Adagrad itself."""
import numpy as np


def adagrad_rule(theta, n, g_hat, eta, eps):
    """One AdaGrad step of arrays (fp64) -> (theta, n)."""
    n = n + g_hat * g_hat
    return theta - eta * g_hat / (np.sqrt(n) + eps), n


def sigmoid(z):
    z = np.asarray(z, np.float64)
    ez = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + ez), ez / (1.0 + ez))


class State:
    """Parameters (w0, w[n1], v[k][n1]) and their accumulators, fp64."""

    def __init__(self, w0, w, v, init):
        self.w0, self.w, self.v = float(w0), np.array(w, np.float64), np.array(v, np.float64)
        self.n0, self.nw, self.nv = float(init), np.full(self.w.shape, float(init)), np.full(self.v.shape, float(init))

    def copy(self):
        s = State(self.w0, self.w, self.v, 0.0)
        s.n0, s.nw, s.nv = self.n0, self.nw.copy(), self.nv.copy()
        return s


def targets(s, rp, col, val, y, loss):
    """The labels the squared-loss oracle needs: y itself, or the logistic pseudo-targets at the current parameters."""
    import oracle
    if loss == "squared":
        return np.asarray(y, np.float64)
    yh = oracle.predict(s.w0, s.w, s.v, rp, col, val)
    return yh - (sigmoid(yh) - (np.asarray(y) > 0))


def g_hats(s, rp, col, val, y, r0, r1, reg0, regw, regv, loss="squared"):
    """-> (g_hat of w0, of w, of v) of the rows [r0, r1)."""
    import oracle
    yt = targets(s, rp, col, val, y, loss)
    gv, gw, g0, _, _ = oracle.batch_grad(s.w0, s.w, s.v, r0, r1, rp, col, np.asarray(val, np.float64), yt)
    b = float(r1 - r0)
    return g0 / b + reg0 * s.w0, np.asarray(gw) / b + regw * s.w, np.asarray(gv) / b + regv * s.v


def step(s, rp, col, val, y, r0, r1, eta, reg0, regw, regv, eps, loss="squared"):
    """One AdaGrad step of the rows [r0, r1) in place; -> s."""
    h0, hw, hv = g_hats(s, rp, col, val, y, r0, r1, reg0, regw, regv, loss)
    t0, s.n0 = adagrad_rule(np.float64(s.w0), np.float64(s.n0), h0, eta, eps)
    s.w0 = float(t0)
    s.w, s.nw = adagrad_rule(s.w, s.nw, hw, eta, eps)
    s.v, s.nv = adagrad_rule(s.v, s.nv, hv, eta, eps)
    return s


def epochs(s, a, batch_rows, orders, eta, reg0, regw, regv, eps, loss="squared"):
    """Epochs of mini-batches of `batch_rows` consecutive rows, visited in orders[e] (None = ascending)."""
    n = len(a["y"])
    nb = (n + batch_rows - 1) // batch_rows
    for order in orders:
        for b in (range(nb) if order is None else order):
            step(s, a["row_ptr"], a["col"], a["val"], a["y"], b * batch_rows, min(n, (b + 1) * batch_rows), eta, reg0, regw, regv, eps, loss)
    return s


def global_batch(shards, j, batch_rows):
    """The global batch of lock-step position j: every rank's batch j, concatenated in rank order -> (rp, col, val, y)."""
    rp, cols, vals, ys = [0], [], [], []
    for d in shards:
        n = len(d["y"])
        lo, hi = min(n, j * batch_rows), min(n, (j + 1) * batch_rows)
        if hi > lo:
            a0, b0 = int(d["row_ptr"][lo]), int(d["row_ptr"][hi])
            cols.append(d["col"][a0:b0])
            vals.append(d["val"][a0:b0].astype(np.float64))
            rp.extend((d["row_ptr"][lo + 1:hi + 1] - a0 + rp[-1]).tolist())
            ys.append(d["y"][lo:hi].astype(np.float64))
    return np.array(rp, np.int64), np.concatenate(cols), np.concatenate(vals), np.concatenate(ys)


def dp_epochs(s, shards, batch_rows, orders, eta, reg0, regw, regv, eps, loss="squared"):
    """Data-parallel epochs: position j's global batch is one step (orders[e]: the positions' order, None = ascending)."""
    steps = max((len(d["y"]) + batch_rows - 1) // batch_rows for d in shards)
    for order in orders:
        for j in (range(steps) if order is None else order):
            rp, col, val, y = global_batch(shards, j, batch_rows)
            step(s, rp, col, val, y, 0, len(y), eta, reg0, regw, regv, eps, loss)
    return s
