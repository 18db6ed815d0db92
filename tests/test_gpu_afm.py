"""The AFM on the device (include/fmhip_afm.h) against the fp64 twin of afm_ref.py: scoring, a softmax over scores above 100, one step
on test_gpu_deepfm.py's shapes, the frozen attention part and determinism, the planted task, the parameters' round trip."""
import copy

import numpy as np
import pytest

import afm_ref as ref
from test_gpu_deepfm import N1, RATES, STEP_SHAPES, score_rows, step_data  # noqa: F401 — DeepFM's rows, shapes and rates
from test_gpu_cin import check_dense, dense_of  # noqa: E402 — its bound on the dense arrays, over afm_ref.State's layers + [u]
from test_gpu_ffm import STEP_N1, f32, fmhip, rowtol, step_rows  # noqa: F401 — the FFM tests' data, fixtures and tolerances
from test_gpu_parity import TOL_G, TOL_Y

pytestmark = pytest.mark.gpu


def start(seed, n1, k, t, init=None, gain=2.0):
    """fp32 values; v and w as DeepFM's start; the attention part at twice its init scale: pre-activations on both sides of the kink."""
    rng = np.random.default_rng(seed)
    return ref.State(f32(0.3), f32(rng.normal(0, 0.3, n1)), f32(rng.normal(0, 0.3, (n1, k))), *[f32(x) for x in ref.dense(rng, k, t, gain)], init=init)


def device_model(fmhip, s, F, hip):
    m = fmhip.AFMModel(s.w.shape[0] - 1, F, s.v.shape[1], len(s.b))
    m.set_params(s.w0, s.w, s.v, s.W, s.b, s.h, s.p)
    hip._set_rule(m)
    return m


def device_state(m, ada):
    s = ref.State(*m.get_params())
    if ada:
        s.n0, s.nw, s.nv, s.nW, s.nb, s.nh, s.np = m.adagrad_state()
    return s


def check_scores(fmhip, m, s, rows, F, counts):
    """Per row TOL_Y on the linear part plus 4 x 1.2e-7 x the twin's first-order forward bound of the AFM term."""
    want, mag, bound = ref.predict(s, rows, F)
    for n in counts:
        yh = m.predict(fmhip.FFMDataSet.from_rows(rows[:n]))
        err, tol = np.abs(yh - want[:n]), TOL_Y * (1.0 + mag[:n]) + 4 * 1.2e-7 * bound[:n]
        print("rows %d: worst err / tol %.3f" % (n, (err / tol).max()))
        assert np.isfinite(yh).all() and (err <= tol).all()


@pytest.mark.parametrize("t", [16, 48, 64])
@pytest.mark.parametrize("F", [1, 2, 5, 17, 48])
@pytest.mark.parametrize("k", [1, 5, 16])
def test_scoring_vs_twin(fmhip, score_rows, k, F, t):
    """Kp = 4, 8, 16; F = 1: no pair; 2: one live M-row in one tile; 17: a second 16-block holding one field, the diagonal tiles partly
    masked; 48: three blocks, skipped tiles.  1, 2, 3 rows: fewer rows than waves; 5, 9: a wave's second and third row; 300: a third
    workgroup with a part-empty tail, the empty row, 64-entry rows, several entries per field."""
    rows = score_rows[F] if F != 2 else ref.random_rows(np.random.default_rng(102), 300, N1, 2, [0, 1, 2, 17, 33, 64, 5])
    s = start(k * 100 + F, N1, k, t)
    m = device_model(fmhip, s, F, fmhip.HipAFM.run())
    assert m.padded_factors == {1: 4, 5: 8, 16: 16}[k]
    check_scores(fmhip, m, s, rows, F, (1, 2, 3, 5, 9, 300))


def test_softmax_with_scores_above_100(fmhip, score_rows):
    """h scaled until the twin's largest score exceeds 100 (exp(s) alone overflows fp32 near 88): finite, inside the same tolerance."""
    F, rows, s = 17, score_rows[17][:65], start(3, N1, 5, 48)
    smax = ref.predict(s, rows, F, full=True)[3].max()
    s.h = f32(s.h * 150.0 / smax).astype(np.float64)
    assert ref.predict(s, rows, F, full=True)[3].max() > 100
    check_scores(fmhip, device_model(fmhip, s, F, fmhip.HipAFM.run()), s, rows, F, (65,))


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
@pytest.mark.parametrize("t", [16, 64])
@pytest.mark.parametrize("shape,src", STEP_SHAPES)
def test_one_step_vs_twin(fmhip, step_rows, shape, src, t, optimizer, loss):
    """The share of units near the kink (afm_ref.py) is asserted on the twin alone, before the device is looked at.  Measured: 0 in all
    64 batches: most fields of these rows are empty, and such a pair's pre-activation is its bias alone, its own sum of |terms|."""
    (F, k), (rows, y) = shape, step_data(step_rows, shape, src)
    ada = optimizer == "adagrad"
    hip = fmhip.HipAFM.run(loss=loss, optimizer=optimizer, adagrad_init=0.1, linear=shape != (3, 4), **RATES)
    m = device_model(fmhip, start(11, STEP_N1, k, t), F, hip)
    ds = fmhip.FFMDataSet.from_rows(rows, y, batch_rows=600)
    for b, (lo, hi) in enumerate(((0, 600), (600, 601))):          # 600 rows: 5 forward workgroups; then the batch of one row
        s0 = device_state(m, ada)
        s1 = copy.deepcopy(s0)
        tch, absg, share = ref.step(s1, rows[lo:hi], y[lo:hi], F, loss=loss, optimizer=optimizer, linear=shape != (3, 4), **RATES)
        print("units near the kink: %.3g of the batch's" % share)
        assert share <= 1e-5
        st = hip.step(m, ds, b)
        assert st["rows"] == hi - lo and st["steps"] == 1 and st["nonfinite"] == 0
        d = device_state(m, ada)
        assert (np.abs((d.v - s0.v) - (s1.v - s0.v)) <= rowtol(s1.v - s0.v)[:, None] + 1.2e-7 * np.abs(s1.v)).all()
        assert (np.abs((d.w - s0.w) - (s1.w - s0.w)) <= TOL_G * max(np.abs(s1.w - s0.w).max(), 1e-9) + 1.2e-7 * np.abs(s1.w)).all()
        assert d.w0 - s0.w0 == pytest.approx(s1.w0 - s0.w0, rel=TOL_G, abs=1.2e-7 * abs(s1.w0) + 1e-9)
        assert np.array_equal(d.v[~tch], s0.v[~tch]) and np.array_equal(d.w[~tch], s0.w[~tch]) and (d.v[tch] != s0.v[tch]).mean() > 0.9
        if ada:
            assert (np.abs((d.nv - s0.nv) - (s1.nv - s0.nv)) <= 2 * rowtol(s1.nv - s0.nv)[:, None] + 3e-7 * s1.nv).all()
            assert (np.abs((d.nw - s0.nw) - (s1.nw - s0.nw)) <= 2 * TOL_G * max(np.abs(s1.nw - s0.nw).max(), 1e-12) + 3e-7 * s1.nw).all()
            assert d.n0 - s0.n0 == pytest.approx(s1.n0 - s0.n0, rel=2 * TOL_G, abs=3e-7 * s1.n0)
            assert np.array_equal(d.nv[~tch], s0.nv[~tch]) and np.array_equal(d.nw[~tch], s0.nw[~tch])
        check_dense(d, s0, s1, absg, RATES["eta"], ada)


def test_a_frozen_attention_part_and_determinism(fmhip, step_rows):
    """attention=False moves no bit of W, b, h, p (v still steps).  Two identical five-batch epochs in a caller's order: identical bits."""
    (F, k), (rows, y) = (7, 5), [x[:301] for x in step_rows[(7, 5)]]
    ds = fmhip.FFMDataSet.from_rows(rows, y, batch_rows=64)          # 4 batches of 64 and one of 45
    hip = fmhip.HipAFM.run(loss="logistic", optimizer="adagrad", adagrad_init=0.1, attention=False, **RATES)
    s = start(12, STEP_N1, k, 48)
    m = device_model(fmhip, s, F, hip)
    hip.learn(m, ds)
    d = device_state(m, True)
    assert all(np.array_equal(a, b) for a, b in zip(dense_of(d), dense_of(s))) and (d.v != s.v).any()
    assert all((n == np.float32(0.1)).all() for n in dense_of(d, True))
    hip = fmhip.HipAFM.run(loss="logistic", optimizer="adagrad", adagrad_init=0.1, **RATES)
    outs = []
    for _ in range(2):
        m = device_model(fmhip, start(12, STEP_N1, k, 48), F, hip)
        hip.learn(m, ds, [3, 0, 4, 2, 1])
        assert hip.last_stats["rows"] == 301 and hip.last_stats["steps"] == 5
        d = device_state(m, True)
        outs.append([d.w0, d.w, d.v, d.n0, d.nw, d.nv] + dense_of(d) + dense_of(d, True))
    assert all(np.array_equal(a, b) for a, b in zip(*outs)) and not np.array_equal(outs[0][6], s.W)


def test_three_epochs_on_the_planted_task(fmhip):
    t = ref.planted()
    _, want_train, want_test = ref.run_planted(t, epochs=3, batch=300)
    (xtr, ytr), (xte, yte) = t["train"], t["test"]
    hip = fmhip.HipAFM.run(loss="logistic", optimizer="adagrad", eta=ref.P_ETA, regv=ref.P_REGV, maxIteration=3, adagrad_init=1.0)
    m = device_model(fmhip, ref.planted_init(t), ref.P_FIELDS, hip)
    train = fmhip.FFMDataSet.from_rows(xtr, ytr, batch_rows=300)
    hip.fit(m, train)
    got_train, got_test = m.computeLogLoss(train), m.computeLogLoss(fmhip.FFMDataSet.from_rows(xte, yte))
    print("train %.8f (twin %.8f), test %.8f (twin %.8f)" % (got_train, want_train, got_test, want_test))
    assert got_train == pytest.approx(want_train, rel=1e-5) and got_test == pytest.approx(want_test, rel=1e-5)


def test_parameters_round_trip(fmhip):
    """F = 17, k = 5 (Kp = 8: three pad slots a row of W and in p), t = 48: the same fp32 values come back, element for element."""
    rng = np.random.default_rng(3)
    m = fmhip.AFMModel(20, 17, 5, 48)
    fmhip.HipAFM.run(optimizer="adagrad")._set_rule(m)
    draw = lambda lo: tuple(f32(rng.uniform(lo, 1, z.shape)) for z in m._zeros())
    p, n = draw(-1), draw(0)
    m.set_params(0.25, *p)
    m.set_adagrad_state(0.5, *n)
    for got, want in ((m.get_params(), (0.25,) + p), (m.adagrad_state(), (0.5,) + n)):
        assert got[0] == want[0] and all(np.array_equal(a, b) for a, b in zip(got[1:], want[1:]))
