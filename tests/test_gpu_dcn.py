"""The low-rank cross network on the device (include/fmhip_dcn.h) against the fp64 twin of dcn_ref.py: scoring over every row tile, Kp,
depth and rank, one step on the shapes of test_gpu_deepfm.py (the untouched parameters bit-identical), the frozen cross part, the
epoch's determinism, three epochs on the planted task, the refusals that need a model."""
import copy

import numpy as np
import pytest

import dcn_ref as ref
from test_gpu_deepfm import N1, RATES, STEP_SHAPES, score_rows, step_data  # noqa: F401 — DeepFM's rows, shapes and rates
from test_gpu_ffm import STEP_N1, f32, fmhip, rowtol, step_rows  # noqa: F401 — the FFM tests' data, fixtures and tolerances
from test_gpu_parity import TOL_G, TOL_Y

pytestmark = pytest.mark.gpu
CROSS = [(1, 16), (2, 48), (3, 256)]


def start(seed, n1, F, k, L, r, init=None):
    """fp32 values; v and w as DeepFM's start, the cross part at its init scale under c_l ~ N(0, 0.3^2)."""
    rng = np.random.default_rng(seed)
    cross, u = ref.dense(rng, F, k, L, r, c_std=0.3)
    return ref.State(f32(0.3), f32(rng.normal(0, 0.3, n1)), f32(rng.normal(0, 0.3, (n1, k))), [tuple(f32(x) for x in t) for t in cross], f32(u), init=init)


def device_model(fmhip, s, hip):
    F = len(s.u) // s.v.shape[1]
    m = fmhip.DCNModel(s.w.shape[0] - 1, F, s.v.shape[1], len(s.cross), s.cross[0][0].shape[1])
    m.set_params(s.w0, s.w, s.v, s.cross, s.u)
    hip._set_rule(m)
    return m


def device_state(m, ada):
    s = ref.State(*m.get_params())
    if ada:
        s.n0, s.nw, s.nv, s.ncross, s.nu = m.adagrad_state()
    return s


def dense_of(s, n=False):
    """The dense parameters (n: their accumulators) as one flat list: V_0, U_0, c_0, ..., u."""
    return [x for t in (s.ncross if n else s.cross) for x in t] + [s.nu if n else s.u]


@pytest.mark.parametrize("L,r", CROSS)
@pytest.mark.parametrize("F", [1, 5, 17, 48])
@pytest.mark.parametrize("k", [1, 5, 16])
def test_scoring_vs_twin(fmhip, score_rows, k, F, L, r):
    """P = F Kp from 4 to 768 (the limit) at every Kp; F = 48, k = 16, r = 256 is the LDS worst case (a 16-row tile of 116 KB), F = 17,
    k = 16 takes 64 rows at r = 16 and 32 at r = 256.  1 row, one row more than each row tile, and 300 rows: a last tile partly empty,
    three workgroups, the empty row, 64-entry rows, several entries per field.  Per row TOL_Y on the linear part plus 4 x 1.2e-7 x the
    twin's first-order forward bound of the cross term (4: the project's allowance for an unknown tile order)."""
    rows = score_rows[F]
    s = start(k * 100 + F, N1, F, k, L, r)
    m = device_model(fmhip, s, fmhip.HipDCN.run())
    assert m.padded_factors == {1: 4, 5: 8, 16: 16}[k]
    want, mag, cmag = ref.predict(s, rows)
    for n in (1, 17, 33, 65, 300):
        yh = m.predict(fmhip.FFMDataSet.from_rows(rows[:n]))
        err, tol = np.abs(yh - want[:n]), TOL_Y * (1.0 + mag[:n]) + 4 * 1.2e-7 * cmag[:n]
        print("rows %d: worst err / tol %.3f" % (n, (err / tol).max()))
        assert (err <= tol).all()


def check_dense(d, s0, s1, absg, eta, ada):
    """test_gpu_deepfm.check_dense's bound on this model's arrays: a relative 1.2e-7 on the parameter and 2e-7 on the change, plus the
    step's sensitivity to the gradient (eta under SGD, eta / sqrt(n') under AdaGrad) times TOL_G of the twin's sum over the rows of
    |terms| / |B|, floored as rowtol floors it by a thousandth of the array's largest such sum."""
    ac, au = absg
    A = [x for t in ac for x in t] + [au]
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
@pytest.mark.parametrize("L,r", CROSS[1:])
@pytest.mark.parametrize("shape,src", STEP_SHAPES)
def test_one_step_vs_twin(fmhip, step_rows, shape, src, L, r, optimizer, loss):
    (F, k), (rows, y) = shape, step_data(step_rows, shape, src)
    ada = optimizer == "adagrad"
    hip = fmhip.HipDCN.run(loss=loss, optimizer=optimizer, adagrad_init=0.1, linear=shape != (3, 4), **RATES)
    m = device_model(fmhip, start(11, STEP_N1, F, k, L, r), hip)
    ds = fmhip.FFMDataSet.from_rows(rows, y, batch_rows=600)
    for b, (lo, hi) in enumerate(((0, 600), (600, 601))):          # 600 rows: 5 forward workgroups, 2 row splits; then the batch of one row
        s0 = device_state(m, ada)
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
def test_a_frozen_cross_part_with_u_zero(fmhip, step_rows, optimizer):
    """cross=False, u = 0, regv = 0: J is 0, so no dense parameter and no v moves by a bit; w and w0 step as the twin's."""
    (F, k), (rows, y), ada = (7, 5), step_rows[(7, 5)], optimizer == "adagrad"
    s = start(11, STEP_N1, F, k, 2, 48)
    s.u[:] = 0.0
    rule = dict(loss="logistic", optimizer=optimizer, eta=0.05, reg0=0.01, regw=0.02, regv=0.0, regd=0.04)
    hip = fmhip.HipDCN.run(cross=False, adagrad_init=0.1, **rule)
    m = device_model(fmhip, s, hip)
    s0 = device_state(m, ada)
    s1 = copy.deepcopy(s0)
    ref.step(s1, rows[:600], y[:600], cross=False, **rule)
    hip.step(m, fmhip.FFMDataSet.from_rows(rows, y, batch_rows=600), 0)
    d = device_state(m, ada)
    assert all(np.array_equal(a, b) for a, b in zip(dense_of(d), dense_of(s0))) and np.array_equal(d.v, s0.v)
    assert (np.abs((d.w - s0.w) - (s1.w - s0.w)) <= TOL_G * np.abs(s1.w - s0.w).max() + 1.2e-7 * np.abs(s1.w)).all() and (d.w != s0.w).any()
    assert d.w0 - s0.w0 == pytest.approx(s1.w0 - s0.w0, rel=TOL_G, abs=1.2e-7 * abs(s1.w0) + 1e-9)


def test_epoch_is_deterministic(fmhip, step_rows):
    """Two identical runs of an epoch over five batches, in an order of the caller's: identical bits in every parameter and accumulator."""
    (F, k), (rows, y) = (7, 5), [x[:301] for x in step_rows[(7, 5)]]
    hip = fmhip.HipDCN.run(loss="logistic", optimizer="adagrad", adagrad_init=0.1, **RATES)
    ds = fmhip.FFMDataSet.from_rows(rows, y, batch_rows=64)          # 4 batches of 64 and one of 45
    outs = []
    for _ in range(2):
        m = device_model(fmhip, start(12, STEP_N1, F, k, 2, 48), hip)
        hip.learn(m, ds, [3, 0, 4, 2, 1])
        assert hip.last_stats["rows"] == 301 and hip.last_stats["steps"] == 5
        d = device_state(m, True)
        outs.append([d.w0, d.w, d.v, d.n0, d.nw, d.nv] + dense_of(d) + dense_of(d, True))
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


def test_three_epochs_on_the_planted_task(fmhip):
    t = ref.planted()
    _, want_train, want_test = ref.run_planted(t, epochs=3, batch=300)
    (xtr, ytr), (xte, yte) = t["train"], t["test"]
    hip = fmhip.HipDCN.run(loss="logistic", optimizer="adagrad", eta=ref.P_ETA, regv=ref.P_REGV, maxIteration=3, adagrad_init=1.0)
    m = device_model(fmhip, ref.planted_init(t), hip)
    train = fmhip.FFMDataSet.from_rows(xtr, ytr, batch_rows=300)
    hip.fit(m, train)
    got_train, got_test = m.computeLogLoss(train), m.computeLogLoss(fmhip.FFMDataSet.from_rows(xte, yte))
    print("train %.8f (twin %.8f), test %.8f (twin %.8f)" % (got_train, want_train, got_test, want_test))
    assert got_train == pytest.approx(want_train, rel=1e-5) and got_test == pytest.approx(want_test, rel=1e-5)


def test_refusals_that_need_a_model(fmhip):
    hip = fmhip.HipDCN.run(optimizer="sgd")
    m = device_model(fmhip, start(1, 9, 3, 4, 1, 16), hip)
    with pytest.raises(RuntimeError, match=r"field id 3, outside the model's \[0, 3\)"):
        m.predict(fmhip.FFMDataSet.from_rows([[(0, 1, 1.0), (3, 2, 1.0)]]))
    with pytest.raises(RuntimeError, match="feature id 9, above the model's num_attribute = 8"):
        hip.step(m, fmhip.FFMDataSet.from_rows([[(0, 9, 1.0)]], np.ones(1)), 0)
    with pytest.raises(RuntimeError, match="under SGD: it has no accumulators"):
        m.adagrad_state()
