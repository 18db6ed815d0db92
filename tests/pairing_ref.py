"""fp64 reference of pairwise ranking (fmhip_model_set_pairing, FMHIP_PAIRING_ADJACENT) for the tests.

Rows 2j and 2j+1 of a batch are one example; the model's loss is applied to their difference:
    d_j = yhat_2j - yhat_2j+1,   dy_j = y_2j - y_2j+1
    squared:   loss_j = (d_j - dy_j)^2 / 2,                         g_j = d_j - dy_j
    logistic:  loss_j = softplus(-d_j) if dy_j > 0 else softplus(d_j),   g_j = sigmoid(d_j) - [dy_j > 0]
    e_2j = g_j,  e_2j+1 = -g_j;   gradient = sum_r e_r h_r(theta);   |B| = the batch's ROW count
(test_host_pairing.py pins g_j to the derivative of loss_j in d_j by central differences).

The gradient comes from the unchanged squared-loss oracle through the pseudo-target trick of test_gpu_logistic.py /
adagrad_ref.py: at y'_r = yhat_r - e_r the oracle's residual yhat_r - y'_r IS e_r, so oracle.batch_grad / oracle.sgd_step /
adagrad_ref.step with y' in place of y give the paired gradient and step; a trajectory recomputes y' before every step."""
import numpy as np

import adagrad_ref


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


def residuals(yhat, y, loss):
    """e over an even number of rows whose pairs are (2j, 2j+1)."""
    yhat, y = np.asarray(yhat, np.float64), np.asarray(y, np.float64)
    assert len(yhat) % 2 == 0 and len(y) == len(yhat)
    g = pair_g(yhat[0::2] - yhat[1::2], y[0::2] - y[1::2], loss)
    e = np.empty(len(yhat))
    e[0::2], e[1::2] = g, -g
    return e


def pseudo_targets(w0, w, v, rp, col, val, y, loss):
    """-> (y' = yhat - e, e, yhat) at these parameters over all rows (pairs never straddle the even batches cut from them)."""
    import oracle
    yh = oracle.predict(w0, w, v, rp, col, np.asarray(val, np.float64))
    e = residuals(yh, y, loss)
    return yh - e, e, yh


def pair_scores(yhat, y):
    """-> (mean pair log-loss, concordance) of the pairs (2j, 2j+1): what fmhip_pair_logloss returns."""
    yhat, y = np.asarray(yhat, np.float64), np.asarray(y, np.float64)
    d, t = yhat[0::2] - yhat[1::2], (y[0::2] - y[1::2]) > 0
    ll = np.where(t, softplus(-d), softplus(d))
    conc = np.where(d == 0, 0.5, ((d > 0) == t).astype(np.float64))
    return float(ll.mean()), float(conc.mean())


def sgd_epochs(a, batch_rows, orders, eta, reg0, regw, regv, loss):
    """Stepped SGD over the even mini-batches of `a`, visited in orders[e] -> (w0, w, v)."""
    import oracle
    w0, w, v = a["w0"], np.array(a["w"], np.float64), np.array(a["v"], np.float64)
    n = len(a["y"])
    nb = (n + batch_rows - 1) // batch_rows
    val = np.asarray(a["val"], np.float64)
    for order in orders:
        for b in (range(nb) if order is None else order):
            r0, r1 = b * batch_rows, min(n, (b + 1) * batch_rows)
            yp, _, _ = pseudo_targets(w0, w, v, a["row_ptr"], a["col"], val, a["y"], loss)
            w0, w, v, _ = oracle.sgd_step(w0, w, v, r0, r1, a["row_ptr"], a["col"], val, yp, eta, reg0, regw, regv)
    return w0, w, v


def adagrad_epochs(s, a, batch_rows, orders, eta, reg0, regw, regv, eps, loss):
    """The same under AdaGrad, on an adagrad_ref.State (in place) -> s."""
    n = len(a["y"])
    nb = (n + batch_rows - 1) // batch_rows
    val = np.asarray(a["val"], np.float64)
    for order in orders:
        for b in (range(nb) if order is None else order):
            yp, _, _ = pseudo_targets(s.w0, s.w, s.v, a["row_ptr"], a["col"], val, a["y"], loss)
            adagrad_ref.step(s, a["row_ptr"], a["col"], val, yp, b * batch_rows, min(n, (b + 1) * batch_rows), eta, reg0, regw, regv, eps,
                             "squared")
    return s


def dp_sgd_epochs(w0, w, v, shards, batch_rows, epochs, eta, reg0, regw, regv, loss):
    """Data-parallel SGD: lock-step position j's global batch (every rank's even batch j, concatenated in rank order) is one step."""
    import oracle
    steps = max((len(d["y"]) + batch_rows - 1) // batch_rows for d in shards)
    w, v = np.array(w, np.float64), np.array(v, np.float64)
    for _ in range(epochs):
        for j in range(steps):
            rp, col, val, y = adagrad_ref.global_batch(shards, j, batch_rows)
            yp, _, _ = pseudo_targets(w0, w, v, rp, col, val, y, loss)
            w0, w, v, _ = oracle.sgd_step(w0, w, v, 0, len(y), rp, col, val, yp, eta, reg0, regw, regv)
    return w0, w, v
