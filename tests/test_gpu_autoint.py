"""AutoInt on the device (include/fmhip_autoint.h) against the fp64 twin of autoint_ref.py: scoring over every token-tile count, Kp,
depth and head shape, the softmax's range, one step on the shapes of test_gpu_deepfm.py (the untouched parameters bit-identical), the
frozen attention part, the epoch's determinism, three epochs on the planted task, the refusals that need a model."""
import copy

import numpy as np
import pytest

import autoint_ref as ref
from test_gpu_deepfm import N1, RATES, STEP_SHAPES, score_rows, step_data  # noqa: F401 — DeepFM's rows, shapes and rates
from test_gpu_ffm import STEP_N1, f32, fmhip, rowtol, step_rows  # noqa: F401 — the FFM tests' data, fixtures and tolerances
from test_gpu_parity import TOL_G, TOL_Y

pytestmark = pytest.mark.gpu
MODELS = [(1, 1, 16), (2, 2, 16), (3, 2, 32), (1, 4, 16)]


def start(seed, n1, F, k, L, H, d, init=None, v_scale=0.3):
    """fp32 values; v and w as DeepFM's start, the attention part at its init scale."""
    rng = np.random.default_rng(seed)
    layers, u = ref.dense(rng, F, k, L, H, d)
    return ref.State(f32(0.3), f32(rng.normal(0, 0.3, n1)), f32(rng.normal(0, v_scale, (n1, k))), [f32(W) for W in layers], f32(u), heads=H, init=init)


def device_model(fmhip, s, hip):
    A = s.layers[0].shape[1] // 4
    m = fmhip.AutoIntModel(s.w.shape[0] - 1, len(s.u) // A, s.v.shape[1], len(s.layers), s.heads, A // s.heads)
    m.set_params(s.w0, s.w, s.v, s.layers, s.u)
    hip._set_rule(m)
    return m


def device_state(m, ada):
    s = ref.State(*m.get_params(), heads=m.heads)
    if ada:
        s.n0, s.nw, s.nv, s.nlayers, s.nu = m.adagrad_state()
    return s


def dense_of(s, n=False):
    """The dense parameters (n: their accumulators) as one flat list: W_0, ..., u."""
    return list(s.nlayers if n else s.layers) + [s.nu if n else s.u]


def check_scores(fmhip, m, s, rows, counts):
    want, mag, cmag = ref.predict(s, rows)
    for n in counts:
        yh = m.predict(fmhip.FFMDataSet.from_rows(rows[:n]))
        err, tol = np.abs(yh - want[:n]), TOL_Y * (1.0 + mag[:n]) + 4 * 1.2e-7 * cmag[:n]
        print("rows %d: worst err / tol %.3f" % (n, (err / tol).max()))
        assert np.isfinite(yh).all() and (err <= tol).all()


@pytest.mark.parametrize("L,H,d", MODELS)
@pytest.mark.parametrize("F", [1, 5, 17, 48])
@pytest.mark.parametrize("k", [1, 5, 16])
def test_scoring_vs_twin(fmhip, score_rows, k, F, L, H, d):
    """F = 1 is a softmax of one token, F = 17 one token past an MFMA tile (the column mask), F = 48 three tiles; (3, 2, 32) keeps the most
    state.  1, 129 and 300 rows: one row past a workgroup, a last workgroup partly empty; the rows hold the empty row, 64-entry rows,
    absent fields and several entries per field.  Per row TOL_Y on the linear part plus 4 x 1.2e-7 x the twin's first-order forward bound
    of the attention term (4: the project's allowance for an unknown tile order)."""
    s = start(k * 100 + F, N1, F, k, L, H, d)
    m = device_model(fmhip, s, fmhip.HipAutoInt.run())
    assert m.padded_factors == {1: 4, 5: 8, 16: 16}[k]
    check_scores(fmhip, m, s, score_rows[F], (1, 129, 300))


def test_softmax_range(fmhip, score_rows):
    """v scaled until the twin's largest |score| is above 90 (asserted): exp of a raw score would overflow fp32 at 88.7.  The device is
    finite and inside the same tolerance only with the row maximum subtracted."""
    s = start(517, N1, 17, 5, 2, 2, 16, v_scale=0.5)
    o = ref.forward(s, score_rows[17])
    scores = [np.abs(Q[:, :, h * 16:(h + 1) * 16] @ K[:, :, h * 16:(h + 1) * 16].transpose(0, 2, 1)).max() for _, Q, K, _, _, _ in o["keep"] for h in range(2)]
    print("largest |score| %.1f" % max(scores))
    assert max(scores) > 90
    check_scores(fmhip, device_model(fmhip, s, fmhip.HipAutoInt.run()), s, score_rows[17], (300,))


def check_dense(d, s0, s1, absg, eta, ada):
    """test_gpu_dcn.check_dense's bound on this model's arrays: 1.2e-7 |theta| + 2e-7 |change| + the step's sensitivity to the gradient
    (eta under SGD, eta / sqrt(n') under AdaGrad) times TOL_G of the twin's sum over the rows of |terms| / |B|, floored as there."""
    aW, au = absg
    for i, (got, a, b, G) in enumerate(zip(dense_of(d), dense_of(s0), dense_of(s1), aW + [au])):
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
@pytest.mark.parametrize("L,H,d", MODELS[1:3])
@pytest.mark.parametrize("shape,src", STEP_SHAPES)
def test_one_step_vs_twin(fmhip, step_rows, shape, src, L, H, d, optimizer, loss):
    """The batch of one row of shape (3, 4) has yhat = 0.28064584 against y = 0.28081707: under the squared loss its residual cancels three
    digits, which is why the twin's |e_r| carries one ulp of the residual's operands (autoint_ref.gradients); the sum of |terms| is otherwise
    the family's sum over the rows of |e_r| |X_l|^T |dY|."""
    (F, k), (rows, y) = shape, step_data(step_rows, shape, src)
    ada = optimizer == "adagrad"
    hip = fmhip.HipAutoInt.run(loss=loss, optimizer=optimizer, adagrad_init=0.1, linear=shape != (3, 4), **RATES)
    m = device_model(fmhip, start(11, STEP_N1, F, k, L, H, d), hip)
    ds = fmhip.FFMDataSet.from_rows(rows, y, batch_rows=600)
    for b, (lo, hi) in enumerate(((0, 600), (600, 601))):          # 600 rows: 5 workgroup partials; then the batch of one row
        s0 = device_state(m, ada)
        s1 = copy.deepcopy(s0)
        t, absg = ref.step(s1, rows[lo:hi], y[lo:hi], loss=loss, optimizer=optimizer, linear=shape != (3, 4), **RATES)
        st = hip.step(m, ds, b)
        assert st["rows"] == hi - lo and st["steps"] == 1 and st["nonfinite"] == 0
        d_ = device_state(m, ada)
        assert (np.abs((d_.v - s0.v) - (s1.v - s0.v)) <= rowtol(s1.v - s0.v)[:, None] + 1.2e-7 * np.abs(s1.v)).all()
        assert (np.abs((d_.w - s0.w) - (s1.w - s0.w)) <= TOL_G * max(np.abs(s1.w - s0.w).max(), 1e-9) + 1.2e-7 * np.abs(s1.w)).all()
        assert d_.w0 - s0.w0 == pytest.approx(s1.w0 - s0.w0, rel=TOL_G, abs=1.2e-7 * abs(s1.w0) + 1e-9)
        assert np.array_equal(d_.v[~t], s0.v[~t]) and np.array_equal(d_.w[~t], s0.w[~t]) and (d_.v[t] != s0.v[t]).mean() > 0.9
        if ada:
            assert (np.abs((d_.nv - s0.nv) - (s1.nv - s0.nv)) <= 2 * rowtol(s1.nv - s0.nv)[:, None] + 3e-7 * s1.nv).all()
            assert (np.abs((d_.nw - s0.nw) - (s1.nw - s0.nw)) <= 2 * TOL_G * max(np.abs(s1.nw - s0.nw).max(), 1e-12) + 3e-7 * s1.nw).all()
            assert d_.n0 - s0.n0 == pytest.approx(s1.n0 - s0.n0, rel=2 * TOL_G, abs=3e-7 * s1.n0)
            assert np.array_equal(d_.nv[~t], s0.nv[~t]) and np.array_equal(d_.nw[~t], s0.nw[~t])
        check_dense(d_, s0, s1, absg, RATES["eta"], ada)


@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
def test_a_frozen_attention_part_with_u_zero(fmhip, step_rows, optimizer):
    """attention=False, u = 0, regv = 0: J is 0, so no dense parameter and no v moves by a bit; w and w0 step as the twin's."""
    (F, k), (rows, y), ada = (7, 5), step_rows[(7, 5)], optimizer == "adagrad"
    s = start(11, STEP_N1, F, k, 2, 2, 16)
    s.u[:] = 0.0
    rule = dict(loss="logistic", optimizer=optimizer, eta=0.05, reg0=0.01, regw=0.02, regv=0.0, regd=0.04)
    hip = fmhip.HipAutoInt.run(attention=False, adagrad_init=0.1, **rule)
    m = device_model(fmhip, s, hip)
    s0 = device_state(m, ada)
    s1 = copy.deepcopy(s0)
    ref.step(s1, rows[:600], y[:600], attention=False, **rule)
    hip.step(m, fmhip.FFMDataSet.from_rows(rows, y, batch_rows=600), 0)
    d = device_state(m, ada)
    assert all(np.array_equal(a, b) for a, b in zip(dense_of(d), dense_of(s0))) and np.array_equal(d.v, s0.v)
    assert (np.abs((d.w - s0.w) - (s1.w - s0.w)) <= TOL_G * np.abs(s1.w - s0.w).max() + 1.2e-7 * np.abs(s1.w)).all() and (d.w != s0.w).any()
    assert d.w0 - s0.w0 == pytest.approx(s1.w0 - s0.w0, rel=TOL_G, abs=1.2e-7 * abs(s1.w0) + 1e-9)


def test_epoch_is_deterministic(fmhip, step_rows):
    """Two identical runs of an epoch over five batches, in an order of the caller's: identical bits in every parameter and accumulator."""
    (F, k), (rows, y) = (7, 5), [x[:301] for x in step_rows[(7, 5)]]
    hip = fmhip.HipAutoInt.run(loss="logistic", optimizer="adagrad", adagrad_init=0.1, **RATES)
    ds = fmhip.FFMDataSet.from_rows(rows, y, batch_rows=64)          # 4 batches of 64 and one of 45
    outs = []
    for _ in range(2):
        m = device_model(fmhip, start(12, STEP_N1, F, k, 2, 2, 16), hip)
        hip.learn(m, ds, [3, 0, 4, 2, 1])
        assert hip.last_stats["rows"] == 301 and hip.last_stats["steps"] == 5
        d = device_state(m, True)
        outs.append([d.w0, d.w, d.v, d.n0, d.nw, d.nv] + dense_of(d) + dense_of(d, True))
    assert all(np.array_equal(a, b) for a, b in zip(*outs))


def test_three_epochs_on_the_planted_task(fmhip):
    t = ref.planted()
    _, want_train, want_test = ref.run_planted(t, epochs=3, batch=300)
    (xtr, ytr), (xte, yte) = t["train"], t["test"]
    hip = fmhip.HipAutoInt.run(loss="logistic", optimizer="adagrad", eta=ref.P_ETA, regv=ref.P_REGV, maxIteration=3, adagrad_init=1.0)
    m = device_model(fmhip, ref.planted_init(t), hip)
    train = fmhip.FFMDataSet.from_rows(xtr, ytr, batch_rows=300)
    hip.fit(m, train)
    got_train, got_test = m.computeLogLoss(train), m.computeLogLoss(fmhip.FFMDataSet.from_rows(xte, yte))
    print("train %.8f (twin %.8f), test %.8f (twin %.8f)" % (got_train, want_train, got_test, want_test))
    assert got_train == pytest.approx(want_train, rel=1e-5) and got_test == pytest.approx(want_test, rel=1e-5)


def test_refusals_that_need_a_model(fmhip):
    hip = fmhip.HipAutoInt.run(optimizer="sgd")
    m = device_model(fmhip, start(1, 9, 3, 4, 1, 1, 16), hip)
    with pytest.raises(RuntimeError, match=r"field id 3, outside the model's \[0, 3\)"):
        m.predict(fmhip.FFMDataSet.from_rows([[(0, 1, 1.0), (3, 2, 1.0)]]))
    with pytest.raises(RuntimeError, match="feature id 9, above the model's num_attribute = 8"):
        hip.step(m, fmhip.FFMDataSet.from_rows([[(0, 9, 1.0)]], np.ones(1)), 0)
    with pytest.raises(RuntimeError, match="under SGD: it has no accumulators"):
        m.adagrad_state()
