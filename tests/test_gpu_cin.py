"""The Compressed Interaction Network on the device (include/fmhip_cin.h) against the fp64 twin of cin_ref.py: scoring over every row
tile, Kp, depth and map count, one step on the shapes of test_gpu_deepfm.py (the untouched parameters bit-identical), the frozen CIN
part, the epoch's determinism, three epochs on the planted task, the parameters' round trip through the device layout."""
import copy

import numpy as np
import pytest

import cin_ref as ref
from test_gpu_deepfm import N1, RATES, STEP_SHAPES, score_rows, step_data  # noqa: F401 — DeepFM's rows, shapes and rates
from test_gpu_ffm import STEP_N1, f32, fmhip, rowtol, step_rows  # noqa: F401 — the FFM tests' data, fixtures and tolerances
from test_gpu_parity import TOL_G, TOL_Y

pytestmark = pytest.mark.gpu
MAPS = [(16,), (48, 32), (128, 128, 128)]


def start(seed, n1, F, k, maps, rows, init=None):
    """fp32 values; v and w as DeepFM's start; W_l at its init scale, then scaled layer by layer so that the twin's X^l over `rows` has
    rms 1 (asserted within [0.1, 10] after the rounding to fp32): a wrong layer then stands well above the tolerance, and the CIN term is
    not lost under the linear part."""
    rng = np.random.default_rng(seed)
    layers, u = ref.dense(rng, F, k, maps)
    s = ref.State(f32(0.3), f32(rng.normal(0, 0.3, n1)), f32(rng.normal(0, 0.3, (n1, k))), layers, f32(u), init=init)
    for l in range(len(maps)):
        s.layers[l] = f32(s.layers[l] / ref.forward(s, rows)["rms"][l]).astype(np.float64)
    rms = ref.forward(s, rows)["rms"]
    assert (rms >= 0.1).all() and (rms <= 10).all(), rms
    return s


def device_model(fmhip, s, hip):
    m = fmhip.CINModel(s.w.shape[0] - 1, s.layers[0].shape[2], s.v.shape[1], [W.shape[0] for W in s.layers])
    m.set_params(s.w0, s.w, s.v, s.layers, s.u)
    hip._set_rule(m)
    return m


def device_state(m, ada):
    s = ref.State(*m.get_params())
    if ada:
        s.n0, s.nw, s.nv, s.nlayers, s.nu = m.adagrad_state()
    return s


def dense_of(s, n=False):
    """The CIN part (n: its accumulators) as one flat list: W_1, ..., W_L, u."""
    return list(s.nlayers if n else s.layers) + [s.nu if n else s.u]


@pytest.mark.parametrize("maps", MAPS)
@pytest.mark.parametrize("F", [1, 5, 17, 48])
@pytest.mark.parametrize("k", [1, 5, 16])
def test_scoring_vs_twin(fmhip, score_rows, k, F, maps):
    """Kp = 4, 8, 16; Fp = 16, 32, 48 with the last MFMA step of a row partly or wholly past F; F = 48, k = 16, (128, 128, 128) is the
    LDS worst case within the limits.  1 row, one row more than each row tile the launcher can choose (1 .. 64), and 300 rows: a last
    tile partly empty, three workgroups, the empty row, 64-entry rows, several entries per field.  Per row TOL_Y on the linear part plus
    4 x 1.2e-7 x the twin's first-order forward bound of the CIN term (4: the project's allowance for an unknown tile order)."""
    rows = score_rows[F]
    s = start(k * 100 + F, N1, F, k, maps, rows)
    m = device_model(fmhip, s, fmhip.HipCIN.run())
    assert m.padded_factors == {1: 4, 5: 8, 16: 16}[k]
    want, mag, cmag = ref.predict(s, rows)
    for n in (1, 2, 3, 5, 9, 17, 33, 65, 300):
        yh = m.predict(fmhip.FFMDataSet.from_rows(rows[:n]))
        err, tol = np.abs(yh - want[:n]), TOL_Y * (1.0 + mag[:n]) + 4 * 1.2e-7 * cmag[:n]
        print("rows %d: worst err / tol %.3f" % (n, (err / tol).max()))
        assert (err <= tol).all()


def check_dense(d, s0, s1, absg, eta, ada):
    """test_gpu_dcn.check_dense's bound on this model's arrays: a relative 1.2e-7 on the parameter and 2e-7 on the change, plus the
    step's sensitivity to the gradient (eta under SGD, eta / sqrt(n') under AdaGrad) times TOL_G of the twin's sum over the rows of
    |terms| / |B|, floored as rowtol floors it by a thousandth of the array's largest such sum."""
    for i, (got, a, b, G) in enumerate(zip(dense_of(d), dense_of(s0), dense_of(s1), absg[0] + [absg[1]])):
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
@pytest.mark.parametrize("maps", MAPS[1:])
@pytest.mark.parametrize("shape,src", STEP_SHAPES)
def test_one_step_vs_twin(fmhip, step_rows, shape, src, maps, optimizer, loss):
    (F, k), (rows, y) = shape, step_data(step_rows, shape, src)
    ada = optimizer == "adagrad"
    hip = fmhip.HipCIN.run(loss=loss, optimizer=optimizer, adagrad_init=0.1, linear=shape != (3, 4), **RATES)
    m = device_model(fmhip, start(11, STEP_N1, F, k, maps, rows[:64]), hip)
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
def test_a_frozen_cin_part_with_u_zero(fmhip, step_rows, optimizer):
    """cin=False, u = 0, regv = 0: J is 0, so no dense parameter and no v moves by a bit; w and w0 step as the twin's."""
    (F, k), (rows, y), ada = (7, 5), step_rows[(7, 5)], optimizer == "adagrad"
    s = start(11, STEP_N1, F, k, (48, 32), rows[:64])
    s.u[:] = 0.0
    rule = dict(loss="logistic", optimizer=optimizer, eta=0.05, reg0=0.01, regw=0.02, regv=0.0, regd=0.04)
    hip = fmhip.HipCIN.run(cin=False, adagrad_init=0.1, **rule)
    m = device_model(fmhip, s, hip)
    s0 = device_state(m, ada)
    s1 = copy.deepcopy(s0)
    ref.step(s1, rows[:600], y[:600], cin=False, **rule)
    hip.step(m, fmhip.FFMDataSet.from_rows(rows, y, batch_rows=600), 0)
    d = device_state(m, ada)
    assert all(np.array_equal(a, b) for a, b in zip(dense_of(d), dense_of(s0))) and np.array_equal(d.v, s0.v)
    assert (np.abs((d.w - s0.w) - (s1.w - s0.w)) <= TOL_G * np.abs(s1.w - s0.w).max() + 1.2e-7 * np.abs(s1.w)).all() and (d.w != s0.w).any()
    assert d.w0 - s0.w0 == pytest.approx(s1.w0 - s0.w0, rel=TOL_G, abs=1.2e-7 * abs(s1.w0) + 1e-9)


def test_epoch_is_deterministic(fmhip, step_rows):
    """Two identical runs of an epoch over five batches, in an order of the caller's: identical bits in every parameter and accumulator."""
    (F, k), (rows, y) = (7, 5), [x[:301] for x in step_rows[(7, 5)]]
    hip = fmhip.HipCIN.run(loss="logistic", optimizer="adagrad", adagrad_init=0.1, **RATES)
    ds = fmhip.FFMDataSet.from_rows(rows, y, batch_rows=64)          # 4 batches of 64 and one of 45
    outs = []
    for _ in range(2):
        m = device_model(fmhip, start(12, STEP_N1, F, k, (48, 32), rows[:64]), hip)
        hip.learn(m, ds, [3, 0, 4, 2, 1])
        assert hip.last_stats["rows"] == 301 and hip.last_stats["steps"] == 5
        d = device_state(m, True)
        outs.append([d.w0, d.w, d.v, d.n0, d.nw, d.nv] + dense_of(d) + dense_of(d, True))
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


def test_three_epochs_on_the_planted_task(fmhip):
    t = ref.planted()
    _, want_train, want_test = ref.run_planted(t, epochs=3, batch=300)
    (xtr, ytr), (xte, yte) = t["train"], t["test"]
    hip = fmhip.HipCIN.run(loss="logistic", optimizer="adagrad", eta=ref.P_ETA, regv=ref.P_REGV, maxIteration=3, adagrad_init=1.0)
    m = device_model(fmhip, ref.planted_init(t), hip)
    train = fmhip.FFMDataSet.from_rows(xtr, ytr, batch_rows=300)
    hip.fit(m, train)
    got_train, got_test = m.computeLogLoss(train), m.computeLogLoss(fmhip.FFMDataSet.from_rows(xte, yte))
    print("train %.8f (twin %.8f), test %.8f (twin %.8f)" % (got_train, want_train, got_test, want_test))
    assert got_train == pytest.approx(want_train, rel=1e-5) and got_test == pytest.approx(want_test, rel=1e-5)


def test_parameters_round_trip(fmhip):
    """F = 17 (two 16-blocks of fields, the second all but empty), k = 5, maps (32, 16): what set_params and set_adagrad_state store comes
    back from get_params and adagrad_state as the same fp32 values, element for element — the device layout's permutation and pads."""
    rng = np.random.default_rng(3)
    m = fmhip.CINModel(20, 17, 5, (32, 16))
    fmhip.HipCIN.run(optimizer="adagrad")._set_rule(m)
    like = m._zeros()
    draw = lambda lo: (f32(rng.uniform(lo, 1, like[0].shape)), f32(rng.uniform(lo, 1, like[1].shape)), [f32(rng.uniform(lo, 1, W.shape)) for W in like[2]],
                       f32(rng.uniform(lo, 1, like[3].shape)))
    p, n = draw(-1), draw(0)
    m.set_params(0.25, *p)
    m.set_adagrad_state(0.5, *n)
    for got, want in ((m.get_params(), (0.25,) + p), (m.adagrad_state(), (0.5,) + n)):
        assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and np.array_equal(got[4], want[4])
        assert all(np.array_equal(a, b) for a, b in zip(got[3], want[3]))
