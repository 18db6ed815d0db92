"""DeepFM on the device (include/fmhip_deepfm.h) against the fp64 twin of deepfm_ref.py: scoring over every row tile, Kp and depth, one
step on the shapes of test_gpu_ffm.py (the untouched parameters bit-identical), the frozen dense part as the plain FM, the epoch's
determinism, three epochs on the planted task, the refusals that need a model."""
import copy

import numpy as np
import pytest

import deepfm_ref as ref
from test_gpu_ffm import STEP_N1, f32, fmhip, rowtol, step_rows  # noqa: F401 — the FFM tests' data, fixtures and tolerances
from test_gpu_fwfm import refit
from test_gpu_parity import TOL_G, TOL_Y

pytestmark = pytest.mark.gpu
N1 = 90
HIDDEN = [(16,), (48, 16), (256, 32, 16)]


def start(seed, n1, F, k, hidden, init=None):
    """fp32 values; unit-scale pre-activations: He-uniform weights under biases ~ N(0, 1)."""
    rng = np.random.default_rng(seed)
    layers, u = ref.dense(rng, F, k, hidden)
    layers = [(f32(W), f32(rng.normal(0, 1, len(b)))) for W, b in layers]
    return ref.State(f32(0.3), f32(rng.normal(0, 0.3, n1)), f32(rng.normal(0, 0.3, (n1, k))), layers, f32(u), init=init)


def device_model(fmhip, s, hip):
    m = fmhip.DeepFMModel(s.w.shape[0] - 1, s.layers[0][0].shape[0] // s.v.shape[1], s.v.shape[1], [len(b) for _, b in s.layers])
    m.set_params(s.w0, s.w, s.v, s.layers, s.u)
    hip._set_rule(m)
    return m


def device_state(m, ada):
    s = ref.State(*m.get_params())
    if ada:
        s.n0, s.nw, s.nv, s.nlayers, s.nu = m.adagrad_state()
    return s


def dense_of(s, n=False):
    """The dense parameters (n: their accumulators) as one flat list: W_1, b_1, ..., u."""
    return [x for pair in (s.nlayers if n else s.layers) for x in pair] + [s.nu if n else s.u]


@pytest.fixture(scope="module")
def score_rows():
    """300 rows per F: the empty row first, lengths up to 64, several entries per field."""
    return {F: ref.random_rows(np.random.default_rng(100 + F), 300, N1, F, [0, 1, 2, 17, 33, 64, 5]) for F in (1, 5, 17, 48)}


@pytest.mark.parametrize("hidden", HIDDEN)
@pytest.mark.parametrize("F", [1, 5, 17, 48])
@pytest.mark.parametrize("k", [1, 5, 16])
def test_scoring_vs_twin(fmhip, score_rows, k, F, hidden):
    """P = F Kp from 4 to 768 (the limit; every combination is inside it), one to three layers; 1 row, one row more than each of the
    three row tiles (16, 32, 64), and 300 rows: a last tile partly empty, three workgroups.  Per row the FmFM scoring test's bound on the
    FM part plus 4 x 1.2e-7 x the dense products' sum of |terms| (the fp32 dot chains' forward bound; 4 for their unknown tile order)."""
    rows = score_rows[F]
    s = start(k * 100 + F, N1, F, k, hidden)
    m = device_model(fmhip, s, fmhip.HipDeepFM.run())
    assert m.padded_factors == {1: 4, 5: 8, 16: 16}[k]
    want, mag, dmag = ref.predict(s, rows)
    for n in (1, 17, 33, 65, 300):
        yh = m.predict(fmhip.FFMDataSet.from_rows(rows[:n]))
        err, tol = np.abs(yh - want[:n]), TOL_Y * (1.0 + mag[:n]) + 4 * 1.2e-7 * dmag[:n]
        print("rows %d: worst err / tol %.3f" % (n, (err / tol).max()))
        assert (err <= tol).all()


# (shape, hidden) -> the seed of the step's starting parameters: the first of 11, 12, ... at which the twin's smallest |pre-activation|
# over the batch of 600 rows is >= 1e-5, found on the CPU (the seeds before it, if any, were tried and put a unit inside that margin)
SEEDS = {((7, 5), (48, 16)): 12, ((7, 5), (256, 32, 16)): 12, ((64, 8), (48, 16)): 11, ((64, 8), (256, 32, 16)): 12, ((3, 4), (48, 16)): 11,
         ((3, 4), (256, 32, 16)): 11, ((39, 16), (48, 16)): 11, ((39, 16), (256, 32, 16)): 15}
STEP_SHAPES = [((7, 5), (7, 5)), ((64, 8), (64, 16)), ((3, 4), (3, 4)), ((39, 16), (7, 5))]
RATES = dict(eta=0.05, reg0=0.01, regw=0.02, regv=0.03, regd=0.04)


def step_data(step_rows, shape, src):
    rows, y = step_rows[src]
    return (refit(rows, [0, 15, 16, 38, 31]) if shape == (39, 16) else rows), y          # (39, 16): the (7, 5) data across the whole width, P = 624


def check_dense(d, s0, s1, absg, eta, ada):
    """A dense parameter's change against the twin's: a relative 1.2e-7 on the parameter and 2e-7 on the change (the step's own fp32
    multiply, square root and divide), plus the step's sensitivity to the gradient — eta under SGD, eta / sqrt(n') under AdaGrad: the
    derivative of g / sqrt(n + g^2) is at most 1 / sqrt(n + g^2) — times the gradient's fp32 error: TOL_G of the twin's sum over the
    rows of |e_r h_{l-1,r} delta_{l,r}| / |B| (600 rows' summation bound 600 x 6e-8 = 3.6e-5, the rest for the terms' own forward error),
    floored as rowtol floors it by a thousandth of the array's largest such sum: the forward error of an h or a delta is relative to
    its dot chain's terms, which the array shares, not to a small h or delta itself."""
    al, au = absg
    A = [x for pair in al for x in pair] + [au]
    for i, (got, a, b, G) in enumerate(zip(dense_of(d), dense_of(s0), dense_of(s1), A)):
        G = TOL_G * np.maximum(G, 1e-3 * G.max())
        sens = eta / np.sqrt(dense_of(s1, True)[i]) if ada else eta
        err, tol = np.abs((got - a) - (b - a)), 1.2e-7 * np.abs(b) + 2e-7 * np.abs(b - a) + sens * G
        print("dense %d: worst err / tol %.3f" % (i, (err / np.maximum(tol, 1e-300)).max()))
        assert (err <= tol).all(), i
        if ada:
            gn, n0, n1 = dense_of(d, True)[i], dense_of(s0, True)[i], dense_of(s1, True)[i]
            g = np.sqrt(n1 - n0)
            assert (np.abs((gn - n0) - (n1 - n0)) <= 2 * g * G + G * G + 3e-7 * n1).all(), i


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
@pytest.mark.parametrize("hidden", HIDDEN[1:])
@pytest.mark.parametrize("shape,src", STEP_SHAPES)
def test_one_step_vs_twin(fmhip, step_rows, shape, src, hidden, optimizer, loss):
    (F, k), (rows, y) = shape, step_data(step_rows, shape, src)
    ada = optimizer == "adagrad"
    hip = fmhip.HipDeepFM.run(loss=loss, optimizer=optimizer, adagrad_init=0.1, linear=shape != (3, 4), **RATES)
    m = device_model(fmhip, start(SEEDS[shape, hidden], STEP_N1, F, k, hidden), hip)
    ds = fmhip.FFMDataSet.from_rows(rows, y, batch_rows=600)
    for b, (lo, hi) in enumerate(((0, 600), (600, 601))):          # 600 rows: 5 forward workgroups, 2 row splits; then the batch of one row
        s0 = device_state(m, ada)
        assert ref.margin(s0, rows[lo:hi]) >= 1e-5          # no pre-activation close enough to 0 for fp32 to flip its mask
        s1 = copy.deepcopy(s0)
        t, absg = ref.step(s1, rows[lo:hi], y[lo:hi], loss=loss, optimizer=optimizer, linear=shape != (3, 4), **RATES)
        st = hip.step(m, ds, b)
        assert st["rows"] == hi - lo and st["steps"] == 1 and st["nonfinite"] == 0
        d = device_state(m, ada)
        assert (np.abs((d.v - s0.v) - (s1.v - s0.v)) <= rowtol(s1.v - s0.v)[:, None] + 1.2e-7 * np.abs(s1.v)).all()
        assert (np.abs((d.w - s0.w) - (s1.w - s0.w)) <= TOL_G * max(np.abs(s1.w - s0.w).max(), 1e-9) + 1.2e-7 * np.abs(s1.w)).all()
        assert d.w0 - s0.w0 == pytest.approx(s1.w0 - s0.w0, rel=TOL_G, abs=1.2e-7 * abs(s1.w0) + 1e-9)
        assert np.array_equal(d.v[~t], s0.v[~t]) and np.array_equal(d.w[~t], s0.w[~t]) and (d.v[t] != s0.v[t]).mean() > 0.9
        if ada:
            assert (np.abs((d.nv - s0.nv) - (s1.nv - s0.nv)) <= 2 * rowtol(s1.nv - s0.nv)[:, None] + 3e-7 * s1.nv).all()
            assert (np.abs((d.nw - s0.nw) - (s1.nw - s0.nw)) <= 2 * TOL_G * max(np.abs(s1.nw - s0.nw).max(), 1e-12) + 3e-7 * s1.nw).all()
            assert d.n0 - s0.n0 == pytest.approx(s1.n0 - s0.n0, rel=2 * TOL_G, abs=3e-7 * s1.n0)
            assert np.array_equal(d.nv[~t], s0.nv[~t]) and np.array_equal(d.nw[~t], s0.nw[~t])
        check_dense(d, s0, s1, absg, RATES["eta"], ada)


@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
def test_a_frozen_dense_part_with_u_zero_is_the_plain_fm(fmhip, step_rows, optimizer):
    """deep=False, u = 0: no dense parameter moves by a bit, and v, w, w0 step as HipFwFM(field_weights=False) steps them at r = 1."""
    (F, k), (rows, y), ada = (7, 5), step_rows[(7, 5)], optimizer == "adagrad"
    s = start(11, STEP_N1, F, k, (48, 16))
    s.u[:] = 0.0
    rule = dict(loss="logistic", optimizer=optimizer, adagrad_init=0.1, eta=0.05, reg0=0.01, regw=0.02, regv=0.03)
    hip = fmhip.HipDeepFM.run(deep=False, regd=0.04, **rule)
    m = device_model(fmhip, s, hip)
    fw, fhip = fmhip.FwFMModel(STEP_N1 - 1, F, k), fmhip.HipFwFM.run(field_weights=False, **rule)
    fw.set_params(s.w0, s.w, s.v, np.ones((F, F)))
    ds = fmhip.FFMDataSet.from_rows(rows, y, batch_rows=600)
    hip.step(m, ds, 0)
    fhip.step(fw, ds, 0)
    d, (w0, w, v, _) = device_state(m, ada), fw.get_params()
    assert all(np.array_equal(a, b) for a, b in zip(dense_of(d), dense_of(s)))
    assert (np.abs(d.v - v) <= rowtol(v - s.v)[:, None] + 1.2e-7 * np.abs(v)).all() and (d.v != s.v).any()
    assert (np.abs(d.w - w) <= TOL_G * np.abs(w - s.w).max() + 1.2e-7 * np.abs(w)).all()
    assert d.w0 - s.w0 == pytest.approx(w0 - s.w0, rel=TOL_G, abs=1.2e-7 * abs(w0) + 1e-9)


def test_epoch_is_deterministic(fmhip, step_rows):
    """Two identical runs of an epoch over five batches, in an order of the caller's: identical bits in every parameter and accumulator."""
    (F, k), (rows, y) = (7, 5), [x[:301] for x in step_rows[(7, 5)]]
    hip = fmhip.HipDeepFM.run(loss="logistic", optimizer="adagrad", adagrad_init=0.1, **RATES)
    ds = fmhip.FFMDataSet.from_rows(rows, y, batch_rows=64)          # 4 batches of 64 and one of 45
    outs = []
    for _ in range(2):
        m = device_model(fmhip, start(12, STEP_N1, F, k, (48, 16)), hip)
        hip.learn(m, ds, [3, 0, 4, 2, 1])
        assert hip.last_stats["rows"] == 301 and hip.last_stats["steps"] == 5
        d = device_state(m, True)
        outs.append([d.w0, d.w, d.v, d.n0, d.nw, d.nv] + dense_of(d) + dense_of(d, True))
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


def test_three_epochs_on_the_planted_task(fmhip):
    t = ref.planted()
    _, want_train, want_test = ref.run_planted(t, epochs=3, batch=300)
    (xtr, ytr), (xte, yte) = t["train"], t["test"]
    hip = fmhip.HipDeepFM.run(loss="logistic", optimizer="adagrad", eta=ref.P_ETA, regv=ref.P_REGV, maxIteration=3, adagrad_init=1.0)
    m = device_model(fmhip, ref.planted_init(t, (64, 32)), hip)
    train = fmhip.FFMDataSet.from_rows(xtr, ytr, batch_rows=300)
    hip.fit(m, train)
    got_train, got_test = m.computeLogLoss(train), m.computeLogLoss(fmhip.FFMDataSet.from_rows(xte, yte))
    print("train %.8f (twin %.8f), test %.8f (twin %.8f)" % (got_train, want_train, got_test, want_test))
    assert got_train == pytest.approx(want_train, rel=1e-5) and got_test == pytest.approx(want_test, rel=1e-5)


def test_refusals_that_need_a_model(fmhip):
    hip = fmhip.HipDeepFM.run(optimizer="sgd")
    m = device_model(fmhip, start(1, 9, 3, 4, (16,)), hip)
    with pytest.raises(RuntimeError, match=r"field id 3, outside the model's \[0, 3\)"):
        m.predict(fmhip.FFMDataSet.from_rows([[(0, 1, 1.0), (3, 2, 1.0)]]))
    with pytest.raises(RuntimeError, match="feature id 9, above the model's num_attribute = 8"):
        hip.step(m, fmhip.FFMDataSet.from_rows([[(0, 9, 1.0)]], np.ones(1)), 0)
    with pytest.raises(RuntimeError, match="under SGD: it has no accumulators"):
        m.adagrad_state()
