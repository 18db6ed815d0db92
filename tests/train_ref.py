"""fp64 reference of every training rule (loss x pairing x optimizer) for the tests, and the fixtures their files share.

The KAT-pinned squared-loss oracle stays as it is; every other residual reaches it through pseudo-targets: at
    y'_r = yhat_r - e_r,   yhat = oracle.predict (fp64)
the oracle's residual yhat_r - y'_r IS e_r, so oracle.batch_grad / oracle.sgd_step with y' in place of y give that rule's
gradient and step; a trajectory recomputes y' before every step.  The residuals:
    single rows   squared: e = yhat - y;   logistic: e = sigmoid(yhat) - [y > 0]
    pairs (rows 2j, 2j+1 of a batch; d_j = yhat_2j - yhat_2j+1, dy_j = y_2j - y_2j+1):   e_2j = g_j,  e_2j+1 = -g_j
        squared:   loss_j = (d_j - dy_j)^2 / 2,                              g_j = d_j - dy_j
        logistic:  loss_j = softplus(-d_j) if dy_j > 0 else softplus(d_j),   g_j = sigmoid(d_j) - [dy_j > 0]
    (test_host_pairing.py pins g_j to the derivative of loss_j in d_j by central differences); |B| = the batch's ROW count.
The update: plain SGD is oracle.sgd_step; AdaGrad, per scalar parameter theta with its accumulator n (torch.optim.Adagrad with
lr = eta, weight_decay = reg, lr_decay = 0; test_host_adagrad.py pins `adagrad_rule` to it):
    g_hat = g/|B| + reg*theta,   n <- n + g_hat^2,   theta <- theta - eta*g_hat / (sqrt(n) + eps)"""
from collections import namedtuple

import numpy as np

# eps None: plain SGD; else AdaGrad with this eps (its initial accumulator is the State's)
Rule = namedtuple("Rule", "loss pairs eps", defaults=("squared", False, None))


def sigmoid(z):
    z = np.asarray(z, np.float64)
    ez = np.exp(-np.abs(z))
    return np.where(z >= 0, 1.0 / (1.0 + ez), ez / (1.0 + ez))


def softplus(z):
    z = np.asarray(z, np.float64)
    return np.maximum(z, 0.0) + np.log1p(np.exp(-np.abs(z)))


def pair_loss(d, dy, loss):
    """The loss of pairs with margins d and targets dy (arrays, fp64)."""
    d, dy = np.asarray(d, np.float64), np.asarray(dy, np.float64)
    if loss == "squared":
        return 0.5 * (d - dy) ** 2
    assert loss == "logistic"
    return np.where(dy > 0, softplus(-d), softplus(d))


def pair_g(d, dy, loss):
    """g_j = d(loss_j)/d(d_j)."""
    d, dy = np.asarray(d, np.float64), np.asarray(dy, np.float64)
    if loss == "squared":
        return d - dy
    assert loss == "logistic"
    return sigmoid(d) - (dy > 0)


def pair_scores(yhat, y):
    """-> (mean pair log-loss, concordance) of the pairs (2j, 2j+1): what fmhip_pair_logloss returns."""
    yhat, y = np.asarray(yhat, np.float64), np.asarray(y, np.float64)
    d, t = yhat[0::2] - yhat[1::2], (y[0::2] - y[1::2]) > 0
    ll = np.where(t, softplus(-d), softplus(d))
    conc = np.where(d == 0, 0.5, ((d > 0) == t).astype(np.float64))
    return float(ll.mean()), float(conc.mean())


def residuals(yhat, y, loss, pairs=False):
    """e of every row; pairs: over an even number of rows whose pairs are (2j, 2j+1)."""
    yhat, y = np.asarray(yhat, np.float64), np.asarray(y, np.float64)
    if not pairs:
        return yhat - y if loss == "squared" else sigmoid(yhat) - (y > 0)
    assert len(yhat) % 2 == 0 and len(y) == len(yhat)
    g = pair_g(yhat[0::2] - yhat[1::2], y[0::2] - y[1::2], loss)
    e = np.empty(len(yhat))
    e[0::2], e[1::2] = g, -g
    return e


def pseudo_targets(w0, w, v, rp, col, val, y, loss, pairs=False):
    """-> (y' = yhat - e, e, yhat) at these parameters over all rows (pairs never straddle the even batches cut from them)."""
    import oracle
    yh = oracle.predict(w0, w, v, rp, col, np.asarray(val, np.float64))
    e = residuals(yh, y, loss, pairs)
    return yh - e, e, yh


def adagrad_rule(theta, n, g_hat, eta, eps):
    """One AdaGrad step of arrays (fp64) -> (theta, n)."""
    n = n + g_hat * g_hat
    return theta - eta * g_hat / (np.sqrt(n) + eps), n


class State:
    """Parameters (w0, w[n1], v[k][n1]) and their accumulators, fp64."""

    def __init__(self, w0, w, v, init=0.0):
        self.w0, self.w, self.v = float(w0), np.array(w, np.float64), np.array(v, np.float64)
        self.n0, self.nw, self.nv = float(init), np.full(self.w.shape, float(init)), np.full(self.v.shape, float(init))

    def copy(self):
        s = State(self.w0, self.w, self.v)
        s.n0, s.nw, s.nv = self.n0, self.nw.copy(), self.nv.copy()
        return s

    def params(self):
        return self.w0, self.w, self.v


def g_hats(s, rp, col, val, y, r0, r1, reg0, regw, regv):
    """-> (g_hat of w0, of w, of v) of the rows [r0, r1) under the squared loss of single rows (y: the rule's targets)."""
    import oracle
    gv, gw, g0, _, _ = oracle.batch_grad(s.w0, s.w, s.v, r0, r1, rp, col, np.asarray(val, np.float64), y)
    b = float(r1 - r0)
    return g0 / b + reg0 * s.w0, np.asarray(gw) / b + regw * s.w, np.asarray(gv) / b + regv * s.v


def step(s, rp, col, val, y, r0, r1, eta, reg0, regw, regv, rule=Rule()):
    """One step of the rows [r0, r1) under `rule`, in place; -> s."""
    import oracle
    val = np.asarray(val, np.float64)
    if rule.loss == "squared" and not rule.pairs:
        yt = np.asarray(y, np.float64)
    else:
        yt = pseudo_targets(s.w0, s.w, s.v, rp, col, val, y, rule.loss, rule.pairs)[0]
    if rule.eps is None:
        s.w0, s.w, s.v, _ = oracle.sgd_step(s.w0, s.w, s.v, r0, r1, rp, col, val, yt, eta, reg0, regw, regv)
        return s
    h0, hw, hv = g_hats(s, rp, col, val, yt, r0, r1, reg0, regw, regv)
    t0, s.n0 = adagrad_rule(np.float64(s.w0), np.float64(s.n0), h0, eta, rule.eps)
    s.w0 = float(t0)
    s.w, s.nw = adagrad_rule(s.w, s.nw, hw, eta, rule.eps)
    s.v, s.nv = adagrad_rule(s.v, s.nv, hv, eta, rule.eps)
    return s


def epochs(s, a, batch_rows, orders, eta, reg0, regw, regv, rule=Rule()):
    """Epochs of mini-batches of `batch_rows` consecutive rows, visited in orders[e] (None = ascending)."""
    n = len(a["y"])
    nb = (n + batch_rows - 1) // batch_rows
    for order in orders:
        for b in (range(nb) if order is None else order):
            step(s, a["row_ptr"], a["col"], a["val"], a["y"], b * batch_rows, min(n, (b + 1) * batch_rows), eta, reg0, regw, regv, rule)
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


def dp_epochs(s, shards, batch_rows, orders, eta, reg0, regw, regv, rule=Rule()):
    """Data-parallel epochs: position j's global batch is one step (orders[e]: the positions' order, None = ascending)."""
    steps = max((len(d["y"]) + batch_rows - 1) // batch_rows for d in shards)
    for order in orders:
        for j in (range(steps) if order is None else order):
            rp, col, val, y = global_batch(shards, j, batch_rows)
            step(s, rp, col, val, y, 0, len(y), eta, reg0, regw, regv, rule)
    return s


# ---- what the GPU test files share: thread-rank shards and their start, comparisons, a dataset with its model -------------

DP_ROWS = {2: [900, 600], 8: [700, 300, 0, 500, 200, 500, 100, 500]}
DP_FRACTIONS = {"dense": (0.3,), "sharded": (0.3,), "touched": (0.3,), "pipelined": (0.1, 0.3, 0.6)}


def dp_shard(seed, rows, rank, all_rows, n1_data, reverse_ids=False, binary=False):
    """Rank `rank`'s rows of a Zipf set; binary: labels {0, 1} split at the shard's median."""
    from sparkfm_amd import synth
    if rows == 0:
        return dict(row_ptr=np.zeros(1, np.int64), col=np.zeros(0, np.int32), val=np.zeros(0, np.float32), y=np.zeros(0, np.float32))
    d = synth.make_zipf(seed, rows, n1_data, 4, 24, zipf_s=1.05, row_begin=int(sum(all_rows[:rank])))
    if reverse_ids:
        d = dict(d, col=(n1_data - 1 - d["col"]).astype(np.int32))
    return dict(d, y=(d["y"] > np.median(d["y"])).astype(np.float32)) if binary else d


def dp_init(n1, k):
    from sparkfm_amd import synth
    w0, w, v = synth.init_params(77, n1, k, stdev=0.05)
    return 0.05, np.random.default_rng(78).normal(0, 0.05, n1), v


def rel(x, y):
    return float(np.linalg.norm(np.asarray(x) - y) / max(np.linalg.norm(y), 1e-30))


def same(x, y):
    return all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(x, y))


def make(fmhip, a, batch_rows=0, hot_block=None, loss="squared"):
    """-> (cached DataSet, FMModel at the problem's parameters, set to `loss`)."""
    from sparkfm_amd import _ffi
    ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=batch_rows, hot_block=hot_block).cache()
    fm = fmhip.FMModel(a["n1"] - 1, a["k"])
    fm.w0, fm.w, fm.v = a["w0"], a["w"], a["v"]
    _ffi.check(_ffi.load().fmhip_model_set_loss(fm.handle, _ffi.loss_code(loss)))
    return ds, fm
