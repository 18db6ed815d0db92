"""The field-weighted FM on the device (include/fmhip_fwfm.h) against the fp64 twin of fwfm_ref.py: scoring over every (Fp, Kp), r = 1 as the
plain FM, one step on the shapes of test_gpu_ffm.py with the untouched parameters bit-identical, the epoch's determinism and order, twenty
epochs on the planted task."""
import copy

import numpy as np
import pytest

import fwfm_ref as ref
from test_gpu_ffm import COUNTS, STEP_N1, f32, fmhip, rowtol, step_rows  # noqa: F401 — the FFM tests' data, fixtures and tolerances
from test_gpu_parity import TOL_G, TOL_Y

pytestmark = pytest.mark.gpu
N1 = 90


def sym(rng, F):
    r = rng.normal(0, 1, (F, F))
    return f32((r + r.T) / 2)


def start(seed, n1, F, k, init=None):
    rng = np.random.default_rng(seed)
    return ref.State(f32(0.3), f32(rng.normal(0, 0.3, n1)), f32(rng.normal(0, 0.3, (n1, k))), sym(rng, F), init=init)


def device_model(fmhip, s, hip):
    m = fmhip.FwFMModel(s.w.shape[0] - 1, s.r.shape[0], s.v.shape[1])
    m.set_params(s.w0, s.w, s.v, s.r)
    hip._set_rule(m)
    return m


def device_state(m, ada):
    s = ref.State(*m.get_params())
    if ada:
        s.n0, s.nw, s.nv, s.nr = m.adagrad_state()
    return s


@pytest.fixture(scope="module")
def score_rows():
    return {F: ref.random_rows(np.random.default_rng(100 + F), 26, N1, F, [0, 1, 2, 17, 33, 64, 5]) for F in (1, 5, 17, 64)}


@pytest.mark.parametrize("F", [1, 5, 17, 64])
@pytest.mark.parametrize("k", [1, 5, 16, 32])
def test_scoring_vs_twin(fmhip, score_rows, k, F):
    rows = score_rows[F]
    s = start(k * 100 + F, N1, F, k)
    m = device_model(fmhip, s, fmhip.HipFwFM.run())
    assert m.padded_factors == {1: 4, 5: 8, 16: 16, 32: 32}[k]
    want, mag = ref.predict(s, rows)
    for batch_rows in (0, 7):
        yh = m.predict(fmhip.FFMDataSet.from_rows(rows, batch_rows=batch_rows))
        assert (np.abs(yh - want) / (1.0 + mag) <= TOL_Y).all()
        assert yh[0] == np.float32(s.w0)          # the empty row


def test_unit_weights_are_the_plain_fm(fmhip, score_rows):
    rows, k = score_rows[5], 5
    s = start(9, N1, 5, k)
    s.r[:] = 1.0
    m = device_model(fmhip, s, fmhip.HipFwFM.run(field_weights=False))
    fm = fmhip.FMModel(N1 - 1, k)
    fm.w0, fm.w, fm.v = s.w0, s.w, s.v.T          # (the FM keeps v as (k, n + 1))
    ptr = np.cumsum([0] + [len(r) for r in rows])
    flat = [e for r in rows for e in r]
    plain = fmhip.DataSet.from_arrays(dict(row_ptr=ptr.astype(np.int64), col=np.array([e[1] for e in flat], np.int32),
                                           val=np.array([e[2] for e in flat], np.float32), y=np.zeros(len(rows), np.float32)))
    got, want = m.predict(fmhip.FFMDataSet.from_rows(rows)), fm.predict(plain)
    assert (np.abs(got - want) / (1.0 + ref.predict(s, rows)[1]) <= TOL_Y).all()


def check_step(m, s0, s1, t, ada):
    """test_gpu_ffm.check_step for this model's parameters; t: the features the batch holds."""
    d = device_state(m, ada)
    assert (np.abs((d.v - s0.v) - (s1.v - s0.v)) <= rowtol(s1.v - s0.v)[:, None] + 1.2e-7 * np.abs(s1.v)).all()
    for name in ("w", "r"):
        got, a, b = getattr(d, name), getattr(s0, name), getattr(s1, name)
        assert (np.abs((got - a) - (b - a)) <= TOL_G * max(np.abs(b - a).max(), 1e-9) + 1.2e-7 * np.abs(b)).all(), name
    assert d.w0 - s0.w0 == pytest.approx(s1.w0 - s0.w0, rel=TOL_G, abs=1.2e-7 * abs(s1.w0) + 1e-9)
    assert np.array_equal(d.r, d.r.T)
    assert np.array_equal(d.v[~t], s0.v[~t]) and np.array_equal(d.w[~t], s0.w[~t]) and (d.v[t] != s0.v[t]).mean() > 0.9
    if ada:
        assert (np.abs((d.nv - s0.nv) - (s1.nv - s0.nv)) <= 2 * rowtol(s1.nv - s0.nv)[:, None] + 3e-7 * s1.nv).all()
        for name in ("nw", "nr"):
            got, a, b = getattr(d, name), getattr(s0, name), getattr(s1, name)
            assert (np.abs((got - a) - (b - a)) <= 2 * TOL_G * max(np.abs(b - a).max(), 1e-12) + 3e-7 * b).all(), name
        assert d.n0 - s0.n0 == pytest.approx(s1.n0 - s0.n0, rel=2 * TOL_G, abs=3e-7 * s1.n0)
        assert np.array_equal(d.nv[~t], s0.nv[~t]) and np.array_equal(d.nw[~t], s0.nw[~t])
    return d


RATES = dict(eta=0.05, reg0=0.01, regw=0.02, regv=0.03, regr=0.04)


def refit(rows, fields):
    """The FFM tests' rows with their field ids mapped onto `fields`, in order of first use."""
    seen = {}
    return [[(fields[seen.setdefault(f, len(seen)) % len(fields)], i, x) for f, i, x in row] for row in rows]


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
@pytest.mark.parametrize("shape,src", [((7, 5), (7, 5)), ((64, 16), (64, 16)), ((3, 4), (3, 4)), ((17, 32), (7, 5))])
def test_one_step_vs_twin(fmhip, step_rows, shape, src, optimizer, loss):
    (F, k), (rows, y) = shape, step_rows[src]
    if shape != src:          # (17, 32): the (7, 5) data on fields of both M tiles
        rows = refit(rows, [0, 15, 16, 3, 9])
    ada = optimizer == "adagrad"
    flags = dict(linear=shape != (3, 4), field_weights=(shape, optimizer) != ((3, 4), "sgd"))
    hip = fmhip.HipFwFM.run(loss=loss, optimizer=optimizer, adagrad_init=0.1, **flags, **RATES)
    m = device_model(fmhip, start(11, STEP_N1, F, k), hip)
    ds = fmhip.FFMDataSet.from_rows(rows, y, batch_rows=600)
    for b, (lo, hi) in enumerate(((0, 600), (600, 601))):          # the batch of 600 rows (5 forward blocks), then the batch of one row
        s0 = device_state(m, ada)
        s1 = copy.deepcopy(s0)
        t = ref.step(s1, rows[lo:hi], y[lo:hi], loss=loss, optimizer=optimizer, **flags, **RATES)
        assert b == 1 or (t[:5].all() and not t[40])
        st = hip.step(m, ds, b)
        assert st["rows"] == hi - lo and st["steps"] == 1 and st["nonfinite"] == 0
        d = check_step(m, s0, s1, t, ada)
        assert flags["linear"] or (d.w0 == s0.w0 and np.array_equal(d.w, s0.w))
        assert flags["field_weights"] or np.array_equal(d.r, s0.r)


def test_a_lone_entry_leaves_its_diagonal_weight(fmhip):
    """Every row holds at most one entry per field: r's diagonal keeps every bit under SGD with regr = 0, and its off-diagonal moves."""
    rng = np.random.default_rng(4)
    F, k = 6, 5
    rows = [[(int(f), int(i), float(rng.normal())) for f, i in zip(rng.choice(F, 4, replace=False), rng.choice(30, 4, replace=False))] for _ in range(300)]
    hip = fmhip.HipFwFM.run(loss="logistic", optimizer="sgd", eta=0.05, regv=0.01)
    s = start(5, 30, F, k)
    m = device_model(fmhip, s, hip)
    hip.step(m, fmhip.FFMDataSet.from_rows(rows, rng.normal(0, 1, 300)), 0)
    r = m.r
    assert np.array_equal(np.diag(r), np.diag(s.r)) and (r != s.r).sum() == F * F - F


def test_an_asymmetric_r_is_refused(fmhip):
    s = start(1, 9, 3, 4)
    m = device_model(fmhip, s, fmhip.HipFwFM.run())
    bad = s.r.copy()
    bad[2, 0] += 0.5
    with pytest.raises(RuntimeError, match=r"r\[0\]\[2\] = .* but r\[2\]\[0\]"):
        m.set_params(s.w0, s.w, s.v, bad)
    assert np.array_equal(m.r, s.r)


def test_epoch_is_deterministic_and_follows_the_order(fmhip, step_rows):
    (F, k), (rows, y) = (7, 5), [x[:301] for x in step_rows[(7, 5)]]
    hip = fmhip.HipFwFM.run(loss="logistic", optimizer="adagrad", adagrad_init=0.1, **RATES)
    ds = fmhip.FFMDataSet.from_rows(rows, y, batch_rows=64)          # 4 batches of 64 and one of 45
    order, outs = [3, 0, 4, 2, 1], []
    for _ in range(2):
        s = start(12, STEP_N1, F, k, init=0.1)
        m = device_model(fmhip, s, hip)
        hip.learn(m, ds, order)
        assert hip.last_stats["rows"] == 301 and hip.last_stats["steps"] == 5
        outs.append(m.get_params() + m.adagrad_state())
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    s0 = copy.deepcopy(s)
    ref.epoch(s, rows, y, 64, order=order, loss="logistic", optimizer="adagrad", **RATES)
    assert (np.abs((outs[0][2] - s0.v) - (s.v - s0.v)) <= rowtol(s.v - s0.v)[:, None] + 1.2e-7 * np.abs(s.v)).all()
    assert (np.abs((outs[0][3] - s0.r) - (s.r - s0.r)) <= TOL_G * np.abs(s.r - s0.r).max() + 1.2e-7 * np.abs(s.r)).all()


def test_twenty_epochs_on_the_planted_task(fmhip):
    t = ref.planted()
    _, want_train, want_test = ref.run_planted(t, 3)
    (xtr, ytr), (xte, yte) = t["train"], t["test"]
    hip = fmhip.HipFwFM.run(loss="logistic", optimizer="adagrad", eta=ref.P_ETA, regv=ref.P_REGV, maxIteration=ref.P_EPOCHS, adagrad_init=1.0)
    m = device_model(fmhip, ref.planted_init(t, 3), hip)
    train = fmhip.FFMDataSet.from_rows(xtr, ytr, batch_rows=ref.P_BATCH)
    hip.fit(m, train)
    got_train, got_test = m.computeLogLoss(train), m.computeLogLoss(fmhip.FFMDataSet.from_rows(xte, yte))
    print("train %.8f (twin %.8f), test %.8f (twin %.8f)" % (got_train, want_train, got_test, want_test))
    assert got_train == pytest.approx(want_train, rel=1e-5) and got_test == pytest.approx(want_test, rel=1e-5)
