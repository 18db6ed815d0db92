"""The field-matrixed FM on the device (include/fmhip_fmfm.h) against the fp64 twin of fmfm_ref.py: scoring over every row tile and Kp up to
the width limit, M = r I as the FwFM and M = I as the plain FM, one step on the shapes of test_gpu_ffm.py (the mirror exact, the diagonal
blocks 0, the untouched parameters bit-identical), the refusals that need a model, the epoch's determinism and order, twenty epochs on
the planted task."""
import copy

import numpy as np
import pytest

import fmfm_ref as ref
from test_gpu_ffm import STEP_N1, f32, fmhip, rowtol, step_rows  # noqa: F401 — the FFM tests' data, fixtures and tolerances
from test_gpu_fwfm import refit, sym
from test_gpu_parity import TOL_G, TOL_Y

pytestmark = pytest.mark.gpu
N1 = 90


def matrices(rng, F, k):
    """(F, F, k, k) as fp32 values: m[g][f] = m[f][g].T, zero diagonal blocks."""
    m = f32(rng.normal(0, 1, (F, F, k, k))) * (np.arange(F)[:, None] < np.arange(F))[:, :, None, None]
    return m + m.transpose(1, 0, 3, 2)


def start(seed, n1, F, k, init=None):
    rng = np.random.default_rng(seed)
    return ref.State(f32(0.3), f32(rng.normal(0, 0.3, n1)), f32(rng.normal(0, 0.3, (n1, k))), matrices(rng, F, k), init=init)


def device_model(fmhip, s, hip):
    m = fmhip.FmFMModel(s.w.shape[0] - 1, s.m.shape[0], s.v.shape[1])
    m.set_params(s.w0, s.w, s.v, s.m)
    hip._set_rule(m)
    return m


def device_state(m, ada):
    s = ref.State(*m.get_params())
    if ada:
        s.n0, s.nw, s.nv, s.nm = m.adagrad_state()
    return s


@pytest.fixture(scope="module")
def score_rows():
    """The FwFM tests' 26 rows per F: the empty row first, lengths up to 64, several entries per field."""
    return {F: ref.random_rows(np.random.default_rng(100 + F), 26, N1, F, [0, 1, 2, 17, 33, 64, 5]) for F in (1, 5, 17, 48)}


@pytest.mark.parametrize("F", [1, 5, 17, 48])
@pytest.mark.parametrize("k", [1, 5, 16])
def test_scoring_vs_twin(fmhip, score_rows, k, F):
    """P = F Kp from 4 (no pair at all) over 20 and 40 (no multiples of 16) to 768 (the limit); row tiles of 64, 32 and 16 rows."""
    rows = score_rows[F]
    s = start(k * 100 + F, N1, F, k)
    m = device_model(fmhip, s, fmhip.HipFmFM.run())
    assert m.padded_factors == {1: 4, 5: 8, 16: 16}[k]
    want, mag = ref.predict(s, rows)
    for batch_rows in (0, 7):
        yh = m.predict(fmhip.FFMDataSet.from_rows(rows, batch_rows=batch_rows))
        assert (np.abs(yh - want) / (1.0 + mag) <= TOL_Y).all()
        assert yh[0] == np.float32(s.w0)          # the empty row


def test_scalar_matrices_are_the_fwfm(fmhip, score_rows):
    rows, F, k = score_rows[5], 5, 5
    s = start(9, N1, F, k)
    r = sym(np.random.default_rng(3), F) * (1 - np.eye(F))
    s.m = r[:, :, None, None] * np.eye(k)
    fw = fmhip.FwFMModel(N1 - 1, F, k)
    fw.set_params(s.w0, s.w, s.v, r)
    ds = fmhip.FFMDataSet.from_rows(rows)
    got, want = device_model(fmhip, s, fmhip.HipFmFM.run(field_matrices=False)).predict(ds), fw.predict(ds)
    assert (np.abs(got - want) / (1.0 + ref.predict(s, rows)[1]) <= TOL_Y).all()


def test_identity_matrices_are_the_plain_fm(fmhip):
    rng = np.random.default_rng(6)
    F, k = 5, 5
    rows = [[(int(f), int(i), float(rng.normal())) for f, i in zip(rng.choice(F, n, replace=False), rng.choice(N1, n, replace=False))] for n in [0, 1, 2, 3, 4, 5] * 5]
    s = start(9, N1, F, k)
    s.m = ref.identity(F, k)
    fm = fmhip.FMModel(N1 - 1, k)
    fm.w0, fm.w, fm.v = s.w0, s.w, s.v.T          # (the FM keeps v as (k, n + 1))
    ptr = np.cumsum([0] + [len(r) for r in rows])
    flat = [e for r in rows for e in r]
    plain = fmhip.DataSet.from_arrays(dict(row_ptr=ptr.astype(np.int64), col=np.array([e[1] for e in flat], np.int32),
                                           val=np.array([e[2] for e in flat], np.float32), y=np.zeros(len(rows), np.float32)))
    got, want = device_model(fmhip, s, fmhip.HipFmFM.run(field_matrices=False)).predict(fmhip.FFMDataSet.from_rows(rows)), fm.predict(plain)
    assert (np.abs(got - want) / (1.0 + ref.predict(s, rows)[1]) <= TOL_Y).all()


def check_step(m, s0, s1, t, ada, joined, regm):
    """test_gpu_fwfm.check_step for v, w, w0; then m: the mirror to the bit, zero diagonal blocks, the blocks of pairs the batch never
    joins (~joined) moved by regm alone."""
    d = device_state(m, ada)
    assert (np.abs((d.v - s0.v) - (s1.v - s0.v)) <= rowtol(s1.v - s0.v)[:, None] + 1.2e-7 * np.abs(s1.v)).all()
    for name in ("w", "m"):
        got, a, b = getattr(d, name), getattr(s0, name), getattr(s1, name)
        assert (np.abs((got - a) - (b - a)) <= TOL_G * max(np.abs(b - a).max(), 1e-9) + 1.2e-7 * np.abs(b)).all(), name
    assert d.w0 - s0.w0 == pytest.approx(s1.w0 - s0.w0, rel=TOL_G, abs=1.2e-7 * abs(s1.w0) + 1e-9)
    assert np.array_equal(d.m, d.m.transpose(1, 0, 3, 2)) and not d.m[np.arange(len(d.m)), np.arange(len(d.m))].any()
    assert regm != 0.0 or np.array_equal(d.m[~joined], s0.m[~joined])
    assert np.array_equal(d.v[~t], s0.v[~t]) and np.array_equal(d.w[~t], s0.w[~t]) and (d.v[t] != s0.v[t]).mean() > 0.9
    if ada:
        assert (np.abs((d.nv - s0.nv) - (s1.nv - s0.nv)) <= 2 * rowtol(s1.nv - s0.nv)[:, None] + 3e-7 * s1.nv).all()
        assert (np.abs((d.nw - s0.nw) - (s1.nw - s0.nw)) <= 2 * TOL_G * max(np.abs(s1.nw - s0.nw).max(), 1e-12) + 3e-7 * s1.nw).all()
        assert (np.abs((d.nm - s0.nm) - (s1.nm - s0.nm)) <= TOL_G * max(np.abs(s1.nm - s0.nm).max(), 1e-12) + 3e-7 * s1.nm).all()
        assert d.n0 - s0.n0 == pytest.approx(s1.n0 - s0.n0, rel=2 * TOL_G, abs=3e-7 * s1.n0)
        assert np.array_equal(d.nv[~t], s0.nv[~t]) and np.array_equal(d.nw[~t], s0.nw[~t]) and np.array_equal(d.nm, d.nm.transpose(1, 0, 3, 2))
        assert regm != 0.0 or np.array_equal(d.nm[~joined], s0.nm[~joined])
    return d


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
@pytest.mark.parametrize("shape,src", [((7, 5), (7, 5)), ((64, 8), (64, 16)), ((3, 4), (3, 4)), ((48, 16), (7, 5))])
def test_one_step_vs_twin(fmhip, step_rows, shape, src, optimizer, loss):
    from sparkfm_amd import _ffi
    (F, k), (rows, y) = shape, step_rows[src]
    if shape == (48, 16):          # the (7, 5) data on fields across the whole width: P = 768
        rows = refit(rows, [0, 15, 16, 47, 31])
    ada = optimizer == "adagrad"
    flags = dict(linear=shape != (3, 4), field_matrices=(shape, optimizer) != ((3, 4), "sgd"))
    rates = dict(eta=0.05, reg0=0.01, regw=0.02, regv=0.03, regm=0.0 if shape == (64, 8) else 0.04)
    hip = fmhip.HipFmFM.run(loss=loss, optimizer=optimizer, adagrad_init=0.1, **flags, **rates)
    m = device_model(fmhip, start(11, STEP_N1, F, k), hip)
    ds = fmhip.FFMDataSet.from_rows(rows, y, batch_rows=600)
    assert 600 > _ffi.FMFM_FORWARD_ROWS and 600 > _ffi.FMFM_GRAD_ROWS          # several forward blocks, several row splits of the gradient
    for b, (lo, hi) in enumerate(((0, 600), (600, 601))):          # the batch of 600 rows, then the batch of one row
        s0 = device_state(m, ada)
        s1 = copy.deepcopy(s0)
        t = ref.step(s1, rows[lo:hi], y[lo:hi], loss=loss, optimizer=optimizer, **flags, **rates)
        assert b == 1 or (t[:5].all() and not t[40])
        joined = np.zeros((F, F), bool)
        for row in rows[lo:hi]:
            fs = [f for f, _, _ in row]
            joined[np.ix_(fs, fs)] = True
        st = hip.step(m, ds, b)
        assert st["rows"] == hi - lo and st["steps"] == 1 and st["nonfinite"] == 0
        d = check_step(m, s0, s1, t, ada, joined, rates["regm"])
        assert flags["linear"] or (d.w0 == s0.w0 and np.array_equal(d.w, s0.w))
        assert flags["field_matrices"] or np.array_equal(d.m, s0.m)


@pytest.mark.parametrize("at,msg", [((2, 0, 1, 3), r"m\[0\]\[2\]\[3\]\[1\] = .* but m\[2\]\[0\]\[1\]\[3\]"), ((1, 1, 2, 0), r"m\[1\]\[1\]\[2\]\[0\] = 0.5")])
def test_a_bad_m_is_refused(fmhip, at, msg):
    """An m that is not mirrored, an m with a non-zero diagonal block: refused with the element named, the model unchanged."""
    s = start(1, 9, 3, 4)
    m = device_model(fmhip, s, fmhip.HipFmFM.run())
    bad = s.m.copy()
    bad[at] += 0.5
    with pytest.raises(RuntimeError, match=msg):
        m.set_params(s.w0 + 1.0, s.w, s.v, bad)
    assert np.array_equal(m.m, s.m) and m.w0 == s.w0


def test_epoch_is_deterministic_and_follows_the_order(fmhip, step_rows):
    (F, k), (rows, y) = (7, 5), [x[:301] for x in step_rows[(7, 5)]]
    rates = dict(eta=0.05, reg0=0.01, regw=0.02, regv=0.03, regm=0.04)
    hip = fmhip.HipFmFM.run(loss="logistic", optimizer="adagrad", adagrad_init=0.1, **rates)
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
    ref.epoch(s, rows, y, 64, order=order, loss="logistic", optimizer="adagrad", **rates)
    assert (np.abs((outs[0][2] - s0.v) - (s.v - s0.v)) <= rowtol(s.v - s0.v)[:, None] + 1.2e-7 * np.abs(s.v)).all()
    assert (np.abs((outs[0][3] - s0.m) - (s.m - s0.m)) <= TOL_G * np.abs(s.m - s0.m).max() + 1.2e-7 * np.abs(s.m)).all()


def test_twenty_epochs_on_the_planted_task(fmhip):
    t = ref.planted()
    _, want_train, want_test = ref.run_planted(t, 3)
    (xtr, ytr), (xte, yte) = t["train"], t["test"]
    hip = fmhip.HipFmFM.run(loss="logistic", optimizer="adagrad", eta=ref.P_ETA, regv=ref.P_REGV, maxIteration=ref.P_EPOCHS, adagrad_init=1.0)
    m = device_model(fmhip, ref.planted_init(t, 3), hip)
    train = fmhip.FFMDataSet.from_rows(xtr, ytr, batch_rows=ref.P_BATCH)
    hip.fit(m, train)
    got_train, got_test = m.computeLogLoss(train), m.computeLogLoss(fmhip.FFMDataSet.from_rows(xte, yte))
    print("train %.8f (twin %.8f), test %.8f (twin %.8f)" % (got_train, want_train, got_test, want_test))
    assert got_train == pytest.approx(want_train, rel=1e-5) and got_test == pytest.approx(want_test, rel=1e-5)
