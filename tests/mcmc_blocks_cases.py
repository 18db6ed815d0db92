"""What the host and the GPU tests of the block-structure MCMC sweep share: the four cases (ungrouped / by parts x regression /
probit), the flat twins' run on the expanded rows, and the twin-to-twin distances measured on the CPU — the yardstick of the GPU
suite's comparison against the flat sampler (test_host_mcmc_relational.py measures them again and holds them to these records)."""
import numpy as np

import mcmc_blocks_ref as B
import mcmc_groups_ref as G
import probit_ref as PR

SEED, EPOCHS = 20251, 3
# (a part is a group, task, sample); without sampling the state is ALS's: alpha = 1, mu = 0, lambda = (REGW, REGV ...), reg0 = REG0
CASES = [(False, "regression", True), (True, "regression", True), (False, "classification", True), (True, "classification", True),
         (False, "regression", False)]
IDS = ["ungrouped", "parts", "probit", "probit-parts", "no-sampling"]
REG0, REGW, REGV = 0.01, 0.1, 5.0
QUANTITIES = ("w", "v", "w0", "alpha", "lambda", "mu", "pred")

# The largest distance between mcmc_blocks_ref and mcmc_groups_ref (+ probit_ref) on expand() after EPOCHS epochs of
# base_problem(SEED): max |a - b| for w, v and the test predictions, max relative for the rest.  Measured on the CPU (numpy, fp64) —
#   ungrouped     w 3.3e-16  v 2.2e-16  w0 0        alpha 0  lambda 2.5e-16  mu 0        pred 2.7e-15
#   parts         w 2.2e-16  v 1.1e-15  w0 0        alpha 0  lambda 2.8e-16  mu 4.9e-14  pred 3.6e-15
#   probit        w 2.2e-16  v 2.4e-16  w0 1.7e-15  alpha 0  lambda 0        mu 9.4e-16  pred 2.2e-16
#   probit-parts  w 2.2e-16  v 3.3e-16  w0 1.9e-14  alpha 0  lambda 1.5e-16  mu 1.1e-15  pred 6.7e-16
#   no-sampling   w 1.8e-15  v 7.2e-16  w0 0        alpha 0  lambda 0        mu 0        pred 5.3e-15
# — and recorded as upper bounds (x4, rounded up; an exact zero as one ulp's worth, 1e-15: another numpy may add in another order).
# Rounding in every case, not a flipped rejection sampler: no seed was changed.
def _rec(w, v, w0, lam, mu, pred):
    return dict(w=w, v=v, w0=w0, alpha=1e-15, **{"lambda": lam}, mu=mu, pred=pred)


RECORDED = dict(zip(CASES, [_rec(2e-15, 1e-15, 1e-15, 1e-15, 1e-15, 2e-14), _rec(1e-15, 5e-15, 1e-15, 2e-15, 2e-13, 2e-14),
                            _rec(1e-15, 1e-15, 7e-15, 1e-15, 4e-15, 1e-15), _rec(1e-15, 2e-15, 8e-14, 1e-15, 5e-15, 3e-15),
                            _rec(8e-15, 3e-15, 1e-15, 1e-15, 1e-15, 3e-14)]))
# what the GPU suite holds the block sweep to against mcmc_blocks_ref (test_gpu_mcmc.py's tolerances for the same arithmetic): w, v
# and predictions absolute + relative, the rest relative — and the floor of the comparison against the flat sampler
TWIN_RTOL, TWIN_ATOL, TWIN_REL = 1e-8, 1e-11, 1e-9


def flat_tolerance(case, quantity):
    """100 x the recorded twin-to-twin distance, floored at the twin-parity tolerance -> (rtol, atol) for w, v, pred; rel otherwise."""
    d = 100.0 * RECORDED[case][quantity]
    return (TWIN_RTOL, max(TWIN_ATOL, d)) if quantity in ("w", "v", "pred") else max(TWIN_REL, d)


def part_of_feature(rp, n1):
    group = np.zeros(n1, np.int64)
    for p, part in enumerate(rp.parts):
        group[part.feat] = p
    return group


def als_state(st):
    st.lam[0], st.lam[1:] = REGW, REGV
    return st


def run_blocks(prob, by_parts, task, sample=True, epochs=EPOCHS, seed=SEED, keep=None):
    """-> the State after `epochs` epochs of the block twin; keep (a list): every epoch's test predictions are appended."""
    rp = prob["train"]
    st = B.State(prob["w0"], prob["w"], prob["v"], n_groups=len(rp.parts) if by_parts else 1)
    if not sample:
        als_state(st)
    for _ in range(epochs):
        B.epoch(st, rp, seed=seed, sample=sample, task=task, reg0=0.0 if sample else REG0)
        if keep is not None:
            yhat = B.predict(st, prob["test"])
            keep.append(PR.normal_cdf(yhat) if task == "classification" else yhat)
    return st


def run_flat(prob, by_parts, task, sample=True, epochs=EPOCHS, seed=SEED):
    """-> the State after `epochs` epochs of the flat twins on the expanded rows."""
    rp = prob["train"]
    flat = rp.expand()
    group = part_of_feature(rp, prob["n1"]) if by_parts else np.zeros(prob["n1"], np.int64)
    st = G.State(prob["w0"], prob["w"], prob["v"], group, len(rp.parts) if by_parts else 1)
    if not sample:
        als_state(st)
    for _ in range(epochs):
        if task == "classification":
            ystar = PR.latent_targets(st, flat, seed, sample)[0]
            G.epoch(st, flat, seed=seed, sample=sample, y=ystar, draw_alpha=False)
        else:
            G.epoch(st, flat, seed=seed, sample=sample, reg0=0.0 if sample else REG0)
    return st


def distances(a, b, pred_a, pred_b):
    """Per quantity the distance between two runs (states with w0, w, v, alpha, lam, mu)."""
    rel = lambda x, y: float(np.max(np.abs(np.asarray(x) - np.asarray(y)) / np.maximum(np.abs(np.asarray(y)), 1e-300)))       # noqa: E731
    return dict(w=float(np.max(np.abs(a.w - b.w))), v=float(np.max(np.abs(a.v - b.v))), w0=rel(a.w0, b.w0), alpha=rel(a.alpha, b.alpha),
                **{"lambda": rel(np.ravel(a.lam), np.ravel(b.lam))}, mu=rel(np.ravel(a.mu), np.ravel(b.mu)), pred=float(np.max(np.abs(pred_a - pred_b))))
