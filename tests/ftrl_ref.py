"""fp64 twin of FTRL-Proximal training (include/fmhip_ftrl.h), built on train_ref.py, and what the FTRL test files share.

Per scalar parameter theta with its states zeta (= alpha * z) and n, and g the plain mean gradient of the batch (nothing folded in):
    g == 0:   theta, zeta, n unchanged
    n' = n + g^2,  r = sqrt(n'),  r0 = sqrt(n),  s = g^2 / (r + r0)  (= r - r0; 0 where r + r0 == 0)
    zeta' = zeta + eta*g - s*theta
    theta' = 0 if |zeta'| <= eta*l1 else -(zeta' - sign(zeta')*eta*l1) / (beta + r + eta*l2)
The gradient comes from the KAT-pinned oracle through train_ref's pseudo-targets (every loss, pairs) and weight_ref's (example
weights), so the twin adds the rule and nothing else.  `dtype=np.float32` runs the same formulas in fp32 on the fp64 gradient
rounded to fp32: what rounding alone may do to the zero pattern (test_host_ftrl.py holds it inside the GPU tests' cap)."""
from collections import namedtuple

import numpy as np

import train_ref as ref
import weight_ref as wref
from test_gpu_parity import TOL_G

# loss, pairs as train_ref.Rule; beta, l1w, l1v: the rule's settings (the accumulators' start is the State's)
Rule = namedtuple("Rule", "loss pairs beta l1w l1v", defaults=("squared", False, 1.0, 0.0, 0.0))


def ftrl_rule(theta, zeta, n, g, eta, l1, l2, beta, dtype=np.float64):
    """One FTRL-Proximal step of arrays -> (theta, zeta, n), in `dtype`."""
    t = dtype
    theta, zeta, n, g = (np.asarray(x, t) for x in (theta, zeta, n, g))
    eta, l1, l2, beta = t(eta), t(l1), t(l2), t(beta)
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        n1 = (g * g + n).astype(t)
        r, r0 = np.sqrt(n1), np.sqrt(n)
        rs = (r + r0).astype(t)
        s = np.where(rs > 0, (g * g).astype(t) / np.where(rs > 0, rs, t(1)), t(0)).astype(t)
        z1 = ((eta * g + zeta).astype(t) - (s * theta).astype(t)).astype(t)
        tau = t(eta * l1)
        den = ((beta + r).astype(t) + t(eta * l2)).astype(t)
        t1 = np.where(np.abs(z1) <= tau, t(0), -(z1 - np.copysign(tau, z1)).astype(t) / den).astype(t)
    moves = g != 0
    return np.where(moves, t1, theta).astype(t), np.where(moves, z1, zeta).astype(t), np.where(moves, n1, n).astype(t)


def zeta_init(theta, n, beta, dtype=np.float64):
    """zeta = -theta * (beta + sqrt(n)): the proximal centre at theta (what fmhip_model_set_ftrl derives)."""
    t = dtype
    return (-np.asarray(theta, t) * (t(beta) + np.sqrt(np.asarray(n, t))).astype(t)).astype(t)


class State:
    """Parameters (w0, w[n1], v[k][n1]) with their zeta and n, in `dtype`; made as fmhip_model_set_ftrl makes the device's."""

    def __init__(self, w0, w, v, init=0.0, beta=1.0, dtype=np.float64):
        t = self.dtype = dtype
        self.w0, self.w, self.v = t(w0), np.array(w, t), np.array(v, t)
        self.n0, self.nw, self.nv = t(init), np.full(self.w.shape, init, t), np.full(self.v.shape, init, t)
        self.z0 = t(zeta_init(self.w0, self.n0, beta, t))
        self.zw, self.zv = zeta_init(self.w, self.nw, beta, t), zeta_init(self.v, self.nv, beta, t)

    def copy(self):
        s = State.__new__(State)
        s.dtype = self.dtype
        for name in ("w0", "n0", "z0"):
            setattr(s, name, getattr(self, name))
        s.g = getattr(self, "g", None)
        for name in ("w", "v", "nw", "nv", "zw", "zv"):
            setattr(s, name, getattr(self, name).copy())
        return s

    def params(self):
        return self.w0, self.w, self.v


def mean_grads(s, rp, col, val, y, r0, r1, rule, c=None):
    """-> (g of w0, of w, of v): the plain mean gradient of the rows [r0, r1) under the rule's loss and pairing (c: example weights),
    fp64 at the state's parameters widened to fp64."""
    val = np.asarray(val, np.float64)
    p = ref.State(float(s.w0), np.asarray(s.w, np.float64), np.asarray(s.v, np.float64))
    if c is not None:
        yt = wref.pseudo_targets(p, rp, col, val, y, c, rule)[0]
    elif rule.loss == "squared" and not rule.pairs:
        yt = np.asarray(y, np.float64)
    else:
        yt = ref.pseudo_targets(p.w0, p.w, p.v, rp, col, val, y, rule.loss, rule.pairs)[0]
    g0, gw, gv = ref.g_hats(p, rp, col, val, yt, r0, r1, 0.0, 0.0, 0.0)
    # pairs: e_2j+1 = -e_2j, so the bias gradient sum e is zero EXACTLY (and the device's is: the two residuals are one number and its
    # negation) — not the rounding noise the oracle's sum of yhat - y' leaves, which the rule would take for a touch (g != 0)
    return (0.0 if rule.pairs else g0), gw, gv


def step(s, rp, col, val, y, r0, r1, eta, l2_0, l2w, l2v, rule=Rule(), c=None):
    """One step of the rows [r0, r1) under `rule`, in place; -> s."""
    g0, gw, gv = s.g = mean_grads(s, rp, col, val, y, r0, r1, rule, c)      # (kept: g != 0 is what "touched" means)
    t = s.dtype
    w0, z0, n0 = ftrl_rule(s.w0, s.z0, s.n0, g0, eta, 0.0, l2_0, rule.beta, t)
    s.w0, s.z0, s.n0 = t(w0), t(z0), t(n0)
    s.w, s.zw, s.nw = ftrl_rule(s.w, s.zw, s.nw, gw, eta, rule.l1w, l2w, rule.beta, t)
    s.v, s.zv, s.nv = ftrl_rule(s.v, s.zv, s.nv, gv, eta, rule.l1v, l2v, rule.beta, t)
    return s


def epochs(s, a, batch_rows, orders, eta, l2_0, l2w, l2v, rule=Rule(), c=None):
    """Epochs of mini-batches of `batch_rows` consecutive rows, visited in orders[e] (None = ascending)."""
    n = len(a["y"])
    nb = (n + batch_rows - 1) // batch_rows
    for order in orders:
        for b in (range(nb) if order is None else order):
            step(s, a["row_ptr"], a["col"], a["val"], a["y"], b * batch_rows, min(n, (b + 1) * batch_rows), eta, l2_0, l2w, l2v, rule, c)
    return s


def dp_epochs(s, shards, batch_rows, orders, eta, l2_0, l2w, l2v, rule=Rule()):
    """Data-parallel epochs: position j's global batch is one step (orders[e]: the positions' order, None = ascending)."""
    steps = max((len(d["y"]) + batch_rows - 1) // batch_rows for d in shards)
    for order in orders:
        for j in (range(steps) if order is None else order):
            rp, col, val, y = ref.global_batch(shards, j, batch_rows)
            step(s, rp, col, val, y, 0, len(y), eta, l2_0, l2w, l2v, rule)
    return s


# ---- what test_host_ftrl.py and test_gpu_ftrl.py share: the one-step problems, the tolerances, the zero pattern's cap -----------

ETA, BETA, INIT = 0.05, 0.5, 0.1
L2 = (1e-3, 2e-3, 3e-3)
KS = [8, 32, 100, 256]          # the packed w slot at Kp 32, k = Kp with a separate w, Kp 128, Kp 256
ZERO_CAP = 0.01                 # coordinates near the L1 threshold, as a share of the touched ones


def problem(seed, n_rows, n1, k, lo, hi, loss):
    """test_gpu_adagrad.py's problems."""
    from helpers import random_problem
    a = random_problem(seed, n_rows, n1, k, lo, hi)
    if loss == "logistic":
        a["y"] = (np.random.default_rng(seed + 1).random(n_rows) < 0.4).astype(np.float64)
    return a


def one_step_problem(k, loss, path):
    """test_gpu_adagrad.py's shapes: dense — 400 rows x 300 features; rows — 150 rows x 6000 features (k_apply_rows).
    The wide problem's rows hold at least TWO entries.  A feature seen only in single-entry rows has the factor gradient
    e x (x v) - v (e x^2): zero in exact arithmetic, rounding noise or exactly zero in floating point, by the order of the products —
    and at g = 0 the rule is discontinuous for a coordinate not yet at its closed form (it does not move; at any g != 0 it takes the
    L1 / L2 shrink of a first touch).  Both answers follow the rule; a twin in another precision cannot say which the device gets, so
    the comparison problems hold no such coordinate (in the 300-feature problem every feature also sits in longer rows)."""
    return problem(40 + k, 400, 300, k, 1, 25, loss) if path == "dense" else problem(60 + k, 150, 6000, k, 2, 12, loss)


def cancelling_features(rp, col, n1):
    """Features seen ONLY in single-entry rows (see one_step_problem): their factor gradient is zero in exact arithmetic.  The
    comparison problems must hold none; the tests assert it."""
    rp, col = np.asarray(rp, np.int64), np.asarray(col, np.int64)
    single = np.repeat(np.diff(rp) == 1, np.diff(rp))
    return np.setdiff1d(np.unique(col[single]), np.unique(col[~single]))


def choose_l1(a, loss, share=0.5):
    """(l1w, l1v) from the twin: the L1 at which `share` of the touched coordinates (g != 0) of one step land on zero — the median
    of |zeta'| / eta over them, so 30-70 % whatever rounding does."""
    s0 = State(a["w0"], a["w"], a["v"], INIT, BETA)
    s1 = step(s0.copy(), a["row_ptr"], a["col"], a["val"], a["y"], 0, len(a["y"]), ETA, *L2, Rule(loss, False, BETA, 0.0, 0.0))
    return float(np.quantile(np.abs(s1.zw[s1.g[1] != 0]), share)) / ETA, float(np.quantile(np.abs(s1.zv[s1.g[2] != 0]), share)) / ETA


def rowtol(d_ref, floor_rel=1e-3):
    """test_gpu_adagrad.rowtol: TOL_G per feature, relative to the largest entry of the feature's column, floored by a thousandth of
    the largest anywhere."""
    scale = max(np.abs(d_ref).max(), 1e-12)
    return TOL_G * np.maximum(np.abs(d_ref).max(axis=0), floor_rel * scale)


def tolerances(s0, s1):
    """check_step's per-feature tolerances (test_gpu_adagrad.py) for the CHANGES s0 -> s1 (fp64 twin states) of theta, zeta and n:
    dict name -> array shaped like the table.  zeta is held as theta is (2 x TOL_G of its feature's largest change + fp32's
    spacing at its value), n as AdaGrad's accumulator."""
    out = {}
    for p, z, n in (("v", "zv", "nv"), ("w", "zw", "nw")):
        for name, ulp in ((p, 1.2e-7), (z, 1.2e-7), (n, 3e-7)):
            d = np.asarray(getattr(s1, name), np.float64) - np.asarray(getattr(s0, name), np.float64)
            if d.ndim == 2:
                tol = 2 * rowtol(d)[None, :]
            else:
                tol = 2 * TOL_G * max(np.abs(d).max(), 1e-9 if name != n else 1e-12)
            out[name] = tol + ulp * np.abs(np.asarray(getattr(s1, name), np.float64))
    return out


def near_threshold(s0, s1, eta, rule):
    """dict "w" / "v" -> bool arrays: the touched coordinates whose twin |zeta'| lies within zeta's tolerance of tau = eta*l1, where
    the device's zero may differ from the twin's."""
    tol = tolerances(s0, s1)
    return {"w": (np.abs(np.abs(s1.zw) - eta * rule.l1w) <= tol["zw"]) & (s1.g[1] != 0),
            "v": (np.abs(np.abs(s1.zv) - eta * rule.l1v) <= tol["zv"]) & (s1.g[2] != 0)}


def planted_task(seed=0, n_feat=200, density=0.1, n_train=4000, n_test=3000, factor_scale=0.4):
    """The end-to-end task: 200 binary features at density 0.1; 20 carry weights +-1.5, the first 8 of them also factors (k = 4,
    N(0, factor_scale)), 180 are noise; click labels drawn from the model's sigmoid.  -> (train, test) dicts of CSR arrays with y in {0, 1}, and the
    informative feature ids."""
    rng = np.random.default_rng(seed)
    info = np.arange(20)
    w = np.zeros(n_feat)
    w[info] = 1.5 * rng.choice([-1.0, 1.0], size=20)
    v = np.zeros((4, n_feat))
    v[:, :8] = rng.normal(0, factor_scale, size=(4, 8))

    def draw(n):
        x = rng.random((n, n_feat)) < density
        x[np.arange(n), rng.integers(0, n_feat, n)] = True          # no empty row
        xf = x.astype(np.float64)
        q = xf @ v.T
        yhat = -0.3 + xf @ w + 0.5 * ((q * q).sum(axis=1) - (xf @ (v * v).T).sum(axis=1))
        y = (rng.random(n) < ref.sigmoid(yhat)).astype(np.float32)
        rp = np.zeros(n + 1, np.int64)
        np.cumsum(x.sum(axis=1), out=rp[1:])
        col = np.nonzero(x)[1].astype(np.int32)
        return dict(row_ptr=rp, col=col, val=np.ones(len(col), np.float32), y=y)

    return draw(n_train), draw(n_test), info
