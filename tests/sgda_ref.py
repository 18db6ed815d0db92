"""The fp64 twin of the SGDA learner (include/fmhip_sgda.h) in plain numpy, and the planted task its tests share.

The rule, per step with a train batch B and a validation batch C (a feature i has the group a = group[i]):
    1. theta' = theta - eta (g_B / |B| + lambda_{a, factor} theta);  w0' = w0 - eta (g_0 / |B| + reg0 w0)
    2. h = the mean gradient of C at theta'
    3. S_w[a] = sum_{i in a} w_i h_w[i],  S_v[f][a] = sum_{i in a} v_{f,i} h_v[f,i]  over the OLD theta;
       lambda <- max(0, lambda + eta_lambda eta S)
Residuals: squared e = yhat - y; logistic e = sigmoid(yhat) - [y > 0] (the library's, include/fmhip.h).  The data is held dense
(the problems here have a few hundred features).  Layouts: w (n1,), v (k, n1), lambda_w (G,), lambda_v (k, G)."""
import numpy as np

ETA, ETA_LAMBDA = 0.05, 0.5
FIXED = (0.0, 0.01, 0.03, 0.1)          # the grid a user of plain SGD would search
EPOCHS, BATCH, K = 150, 50, 4
SEEDS = (3, 4)


def dense(rp, col, val, n1):
    """CSR -> a dense fp64 matrix (rows, n1); a feature stored twice in a row adds up."""
    rp = np.asarray(rp, np.int64)
    X = np.zeros((len(rp) - 1, n1))
    np.add.at(X, (np.repeat(np.arange(len(rp) - 1), np.diff(rp)), np.asarray(col, np.int64)), np.asarray(val, np.float64))
    return X


def csr(X):
    """A dense matrix -> (row_ptr int64, col int32, val fp64) of its nonzeros, ids ascending in a row."""
    rows, cols = np.nonzero(X)
    rp = np.zeros(X.shape[0] + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=X.shape[0]), out=rp[1:])
    return rp, cols.astype(np.int32), X[rows, cols].astype(np.float64)


def predict(w0, w, v, X):
    q = X @ v.T
    return w0 + X @ w + 0.5 * ((q * q) - (X * X) @ (v * v).T).sum(1), q


def residual(yhat, y, loss):
    if loss == "squared":
        return yhat - y
    return 1.0 / (1.0 + np.exp(-yhat)) - (y > 0)


def logloss(yhat, y):
    t = (y > 0).astype(np.float64)
    return float(np.mean(np.logaddexp(0.0, yhat) - t * yhat))


def rmse(yhat, y):
    return float(np.sqrt(np.mean((yhat - y) ** 2)))


def gradient(w0, w, v, X, y, loss):
    """-> (e, g_0, G_w (n1,), G_V (k, n1), G_b (n1,)): the SUMS over the rows, as the packed gradient holds them —
    g of v_{f,i} is G_V[f,i] - v[f,i] G_b[i]."""
    yhat, q = predict(w0, w, v, X)
    e = residual(yhat, y, loss)
    return e, float(e.sum()), X.T @ e, (X * e[:, None]).T.dot(q).T, (X * X).T @ e


class State:
    def __init__(self, w0, w, v, n_groups=1, lambda_w=0.0, lambda_v=0.0):
        self.w0, self.w, self.v = float(w0), np.array(w, np.float64), np.array(v, np.float64)
        k = self.v.shape[0]
        self.lw = np.broadcast_to(np.asarray(lambda_w, np.float64), (n_groups,)).copy()
        self.lv = np.broadcast_to(np.asarray(lambda_v, np.float64), (k, n_groups)).copy()
        self.steps = 0

    def copy(self):
        s = State(self.w0, self.w, self.v, len(self.lw), self.lw, self.lv)
        s.steps = self.steps
        return s


def step(s, group, Xb, yb, Xc, yc, eta, eta_lambda, reg0=0.0, loss="squared"):
    """One step in place.  Xc None: steps 2 and 3 are skipped.  -> dict: e_train; with a validation batch also e_val, S_w (G,),
    S_v (k, G) and T_w, T_v — the sums of the terms' absolute values, the scale the fp32 sums' error is measured against."""
    G = len(s.lw)
    group = np.asarray(group, np.int64)
    e, g0, gw, GV, Gb = gradient(s.w0, s.w, s.v, Xb, yb, loss)
    b = float(len(yb))
    w_old, v_old = s.w, s.v
    s.w0 = s.w0 - eta * (g0 / b + reg0 * s.w0)
    s.w = w_old - eta * (gw / b + s.lw[group] * w_old)
    s.v = v_old - eta * ((GV - v_old * Gb) / b + s.lv[:, group] * v_old)
    out = dict(e_train=e)
    if Xc is not None:
        ec, _, hw, HV, Hb = gradient(s.w0, s.w, s.v, Xc, yc, loss)
        c = float(len(yc))
        tw, tv = w_old * hw / c, v_old * (HV - s.v * Hb) / c
        S_w, T_w = np.zeros(G), np.zeros(G)
        S_v, T_v = np.zeros((len(s.v), G)), np.zeros((len(s.v), G))
        np.add.at(S_w, group, tw)
        np.add.at(T_w, group, np.abs(tw))
        np.add.at(S_v.T, group, tv.T)
        np.add.at(T_v.T, group, np.abs(tv).T)
        s.lw = np.maximum(0.0, s.lw + eta_lambda * eta * S_w)
        s.lv = np.maximum(0.0, s.lv + eta_lambda * eta * S_v)
        out.update(e_val=ec, S_w=S_w, S_v=S_v, T_w=T_w, T_v=T_v)
    s.steps += 1
    return out


def epoch(s, group, X, y, Xv, yv, batch, eta, eta_lambda, reg0=0.0, loss="squared", order=None):
    """The train batches in `order` (None: ascending); step t takes validation batch t mod n_val_batches, t running on over
    epochs in s.steps.  -> (sum e^2 over the train batches, sum e^2 and rows over the validation batches used)."""
    nb = (len(y) + batch - 1) // batch
    nvb = (len(yv) + batch - 1) // batch if Xv is not None else 0
    sse, vsse, vrows = 0.0, 0.0, 0
    for j in (range(nb) if order is None else order):
        r0, r1 = j * batch, min(len(y), (j + 1) * batch)
        if Xv is not None:
            vb = s.steps % nvb
            c0, c1 = vb * batch, min(len(yv), (vb + 1) * batch)
            out = step(s, group, X[r0:r1], y[r0:r1], Xv[c0:c1], yv[c0:c1], eta, eta_lambda, reg0, loss)
            vsse += float((out["e_val"] ** 2).sum())
            vrows += c1 - c0
        else:
            out = step(s, group, X[r0:r1], y[r0:r1], None, None, eta, 0.0, reg0, loss)
        sse += float((out["e_train"] ** 2).sum())
    return sse, vsse, vrows


def sgd_epoch(w0, w, v, X, y, batch, eta, reg0, regw, regv, loss="squared"):
    """Plain fp64 mini-batch SGD with scalar regularisers, written out on its own (what the twin at eta_lambda = 0 must equal)."""
    for r0 in range(0, len(y), batch):
        Xb, yb = X[r0:r0 + batch], y[r0:r0 + batch]
        _, g0, gw, GV, Gb = gradient(w0, w, v, Xb, yb, loss)
        b = float(len(yb))
        w0, w, v = w0 - eta * (g0 / b + reg0 * w0), w - eta * (gw / b + regw * w), v - eta * ((GV - v * Gb) / b + regv * v)
    return w0, w, v


# ---- the planted task ----------------------------------------------------------------------------------------------------------

N_FEAT, N_INF, N_FACT, DENSITY = 200, 20, 8, 0.1
N_TRAIN, N_VAL, N_TEST = 400, 200, 2000


def planted(seed, loss="squared"):
    """200 binary features at density 0.1: ids 0..19 informative (a weight each; 0..7 also interact through rank-2 factors), ids
    20..199 noise.  400 train, 200 validation, 2000 test rows.  The model has num_attribute = 200, so n1 = 201 rows: the spare row
    joins the noise group.  logistic: the labels cut at the train set's median.  Values are exactly representable in fp32."""
    rng = np.random.default_rng([20261021, seed])
    n1 = N_FEAT + 1
    wt = np.zeros(n1)
    wt[:N_INF] = rng.normal(0.0, 1.0, N_INF)
    vt = np.zeros((2, n1))
    vt[:, :N_FACT] = rng.normal(0.0, 1.0, (2, N_FACT))
    parts = {}
    for name, rows in (("train", N_TRAIN), ("val", N_VAL), ("test", N_TEST)):
        X = np.zeros((rows, n1))
        X[:, :N_FEAT] = rng.random((rows, N_FEAT)) < DENSITY
        y = predict(0.5, wt, vt, X)[0] + rng.normal(0.0, 0.3, rows)
        parts[name] = (X, y.astype(np.float32).astype(np.float64))
    if loss == "logistic":
        cut = np.median(parts["train"][1])
        parts = {name: (X, (y > cut).astype(np.float64)) for name, (X, y) in parts.items()}
    group = np.ones(n1, np.int32)
    group[:N_INF] = 0
    v0 = rng.normal(0.0, 0.1, (K, n1)).astype(np.float32).astype(np.float64)
    return dict(n1=n1, k=K, group=group, w0=0.0, w=np.zeros(n1), v=v0, **parts)


def run_planted(task, group, n_groups, eta_lambda, init_lambda=0.0, loss="squared", epochs=EPOCHS, validation=True):
    """The twin's run on a planted task -> (state, validation loss of the last epoch's validation batches, test loss): RMSE, or
    the log-loss under the logistic loss."""
    s = State(task["w0"], task["w"], task["v"], n_groups, init_lambda, init_lambda)
    (X, y), (Xv, yv), (Xt, yt) = task["train"], task["val"], task["test"]
    vsse = vrows = 0
    for _ in range(epochs):
        _, vsse, vrows = epoch(s, group, X, y, Xv if validation else None, yv, BATCH, ETA, eta_lambda, 0.0, loss)
    yhat = predict(s.w0, s.w, s.v, Xt)[0]
    return s, (float(np.sqrt(vsse / vrows)) if vrows else float("nan")), (rmse(yhat, yt) if loss == "squared" else logloss(yhat, yt))
