"""fp64 twin of weighted training (include/fmhip_weights.h), built on train_ref.py.

A dataset carries one weight c_r >= 0 per row and every rule's residual becomes e_r <- c_r * e_r(loss); under pairing the pair's
weight is row 2j's (e_2j = c_2j g_j, e_2j+1 = -c_2j g_j).  |B| stays the batch's ROW count, so the step is the gradient step of
    (1/|B|) sum_r c_r loss_r            (pairs: (1/|B|) sum_j c_2j loss_j)
which test_host_weights.py pins by central differences.  No new oracle: at pseudo-targets y'_r = yhat_r - c_r e_r the KAT-pinned
squared-loss oracle's residual IS the weighted residual — the device train_ref.py uses for every other rule."""
import numpy as np

import train_ref as ref
from train_ref import Rule, State  # noqa: F401 — re-exported for the test files

WEIGHT_VALUES = np.array([0.0, 0.25, 1.0, 3.5])


def draw_weights(seed, n):
    """n weights from {0, 0.25, 1, 3.5}, about a fifth of them 0."""
    return np.random.default_rng(seed).choice(WEIGHT_VALUES, size=n, p=[0.2, 0.3, 0.25, 0.25])


def row_weights(c, pairs):
    """The weight every row's residual is scaled by: its own; under pairing row 2j's for both rows of the pair."""
    c = np.asarray(c, np.float64)
    return np.repeat(c[0::2], 2) if pairs else c


def weighted_residuals(yhat, y, c, loss, pairs=False):
    return row_weights(c, pairs) * ref.residuals(yhat, y, loss, pairs)


def objective(w0, w, v, rp, col, val, y, c, r0, r1, loss, pairs=False):
    """(1/|B|) sum c * loss over the rows [r0, r1) (|B| = r1 - r0 rows; pairs: one term per pair, weighted by row 2j's c)."""
    import oracle
    yh = oracle.predict(w0, w, v, rp, col, np.asarray(val, np.float64))[r0:r1]
    yy, cc = np.asarray(y, np.float64)[r0:r1], np.asarray(c, np.float64)[r0:r1]
    if pairs:
        terms = cc[0::2] * ref.pair_loss(yh[0::2] - yh[1::2], yy[0::2] - yy[1::2], loss)
    elif loss == "squared":
        terms = cc * 0.5 * (yh - yy) ** 2
    else:
        terms = cc * (ref.softplus(yh) - (yy > 0) * yh)
    return float(terms.sum()) / float(r1 - r0)


def pseudo_targets(s, rp, col, val, y, c, rule):
    """-> (y' = yhat - c e, c e, yhat) over all rows at the state's parameters."""
    import oracle
    yh = oracle.predict(s.w0, s.w, s.v, rp, col, np.asarray(val, np.float64))
    e = weighted_residuals(yh, y, c, rule.loss, rule.pairs)
    return yh - e, e, yh


def step(s, rp, col, val, y, c, r0, r1, eta, reg0, regw, regv, rule=Rule()):
    """One weighted step of the rows [r0, r1) under `rule`, in place; -> s.  (train_ref.step at the weighted pseudo-targets,
    taken as the squared loss of single rows.)"""
    yt = pseudo_targets(s, rp, col, val, y, c, rule)[0]
    return ref.step(s, rp, col, np.asarray(val, np.float64), yt, r0, r1, eta, reg0, regw, regv, Rule("squared", False, rule.eps))


def epochs(s, a, c, batch_rows, orders, eta, reg0, regw, regv, rule=Rule()):
    """Weighted epochs of mini-batches of `batch_rows` consecutive rows, visited in orders[e] (None = ascending)."""
    n = len(a["y"])
    nb = (n + batch_rows - 1) // batch_rows
    for order in orders:
        for b in (range(nb) if order is None else order):
            step(s, a["row_ptr"], a["col"], a["val"], a["y"], c, b * batch_rows, min(n, (b + 1) * batch_rows), eta, reg0, regw, regv, rule)
    return s


def global_weights(shards, j, batch_rows):
    """The weights of lock-step position j's global batch, in train_ref.global_batch's row order (a shard without "weights": ones)."""
    out = []
    for d in shards:
        n = len(d["y"])
        lo, hi = min(n, j * batch_rows), min(n, (j + 1) * batch_rows)
        if hi > lo:
            out.append(np.asarray(d["weights"], np.float64)[lo:hi] if d.get("weights") is not None else np.ones(hi - lo))
    return np.concatenate(out)


def dp_epochs(s, shards, batch_rows, orders, eta, reg0, regw, regv, rule=Rule()):
    """Data-parallel weighted epochs: position j's global batch is one step."""
    steps = max((len(d["y"]) + batch_rows - 1) // batch_rows for d in shards)
    for order in orders:
        for j in (range(steps) if order is None else order):
            rp, col, val, y = ref.global_batch(shards, j, batch_rows)
            step(s, rp, col, val, y, global_weights(shards, j, batch_rows), 0, len(y), eta, reg0, regw, regv, rule)
    return s


def weighted_scores(yhat, y, c):
    """What fmhip_weighted_scores returns, in fp64 numpy: dict of sum_w, rmse, mae, logloss (nan ratios when sum c == 0)."""
    yhat, y, c = (np.asarray(x, np.float64) for x in (yhat, y, c))
    sw = float(c.sum())
    if not sw > 0:
        return dict(sum_w=sw, rmse=float("nan"), mae=float("nan"), logloss=float("nan"))
    keep = c > 0
    d = (yhat - y)[keep]
    ll = (ref.softplus(yhat) - (y > 0) * yhat)[keep]
    return dict(sum_w=sw, rmse=float(np.sqrt((c[keep] * d * d).sum() / sw)), mae=float((c[keep] * np.abs(d)).sum() / sw),
                logloss=float((c[keep] * ll).sum() / sw))
