"""The field-aware FM on the device (include/fmhip_ffm.h) against the fp64 twin of ffm_ref.py: scoring, one step on the shapes where the
column walk can go wrong with the untouched parameters bit-identical, the epoch's determinism and order, twenty epochs on the planted task."""
import copy

import numpy as np
import pytest

import ffm_ref as ref
from test_gpu_parity import TOL_G, TOL_Y

pytestmark = pytest.mark.gpu

f32 = lambda x: np.asarray(x, np.float32).astype(np.float64)          # noqa: E731 — the device holds fp32
N1 = 90          # the scoring tests' feature rows


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def device_model(fmhip, s, F, k, hip):
    m = fmhip.FFMModel(s.w.shape[0] - 1, F, k)
    m.set_params(s.w0, s.w, s.v)
    hip._set_rule(m)
    return m


def start(seed, n1, F, k, init=None):
    rng = np.random.default_rng(seed)
    return ref.State(f32(0.3), f32(rng.normal(0, 0.3, n1)), f32(rng.normal(0, 0.3, (n1, F, k))), init=init)


@pytest.fixture(scope="module")
def score_rows():
    """Per F: 26 rows of 0, 1, 2, 17, 33, 64 and 5 entries (ffm_ref.random_rows: runs longer than 1, a row of one field, ids 0 and n, a zero)."""
    return {F: ref.random_rows(np.random.default_rng(100 + F), 26, N1, F, [0, 1, 2, 17, 33, 64, 5]) for F in (1, 2, 5, 64)}


@pytest.mark.parametrize("F", [1, 2, 5, 64])
@pytest.mark.parametrize("k", [1, 4, 5, 16])
def test_scoring_vs_twin(fmhip, score_rows, k, F):
    rows = score_rows[F]
    s = start(k * 100 + F, N1, F, k)
    m = device_model(fmhip, s, F, k, fmhip.HipFFM.run())
    assert m.padded_factors == {1: 4, 4: 4, 5: 8, 16: 16}[k]
    for batch_rows in (0, 7):
        ds = fmhip.FFMDataSet.from_rows(rows, batch_rows=batch_rows)
        assert ds.info()["max_row"] == 64 and ds.n_batches == (1 if batch_rows == 0 else 4)
        yh = m.predict(ds)
        want, mag = ref.predict(s, rows)
        err = np.abs(yh - want) / (1.0 + mag)
        assert (err <= TOL_Y).all()
        assert yh[0] == np.float32(s.w0)          # the empty row


STEP_N1 = 41          # (the data holds feature ids below 40: a row nothing touches)
# (F, k) -> the fields the data uses (row 0 the first two): Kp = 8, 16 and 4; both words of the touched-fields mask; fields nothing touches
SHAPES = {(7, 5): [0, 1, 2, 3, 4], (64, 16): [33, 2, 31, 32, 47, 63], (3, 4): [0, 2]}
COUNTS = {0: 600, 1: 257, 2: 256, 3: 255, 4: 1}          # feature -> the rows of batch 0 that hold it


@pytest.fixture(scope="module")
def step_rows():
    """Per shape 601 rows in batches of 600 and 1: batch 0 holds features 0 .. 4 in COUNTS of its rows; 2 .. 4 other features a row."""
    out = {}
    for shape, used in SHAPES.items():
        rng = np.random.default_rng(5)
        rows = []
        for r in range(601):
            feats = [i for i, c in COUNTS.items() if r < c] + rng.choice(np.arange(5, 40), int(rng.integers(2, 5)), replace=False).tolist()
            rows.append([(used[int(rng.integers(len(used) if r else 2))], int(i), float(rng.normal())) for i in feats])
        out[shape] = rows, rng.normal(0, 1, 601)
    return out


def rowtol(d_ref):
    """TOL_G per feature row: of the row's largest change, floored by a thousandth of the largest anywhere (test_gpu_adagrad.py)."""
    flat = np.abs(d_ref).reshape(d_ref.shape[0], -1)
    return TOL_G * np.maximum(flat.max(axis=1), 1e-3 * max(flat.max(), 1e-12))


def device_state(m, ada):
    s = ref.State(*m.get_params())
    if ada:
        s.n0, s.nw, s.nv = m.adagrad_state()
    return s


def check_step(m, s0, s1, tv, tw, ada):
    d = device_state(m, ada)
    tol = rowtol(s1.v - s0.v)[:, None, None] + 1.2e-7 * np.abs(s1.v)
    dv = (d.v - s0.v) - (s1.v - s0.v)
    assert (np.abs(dv) <= tol).all()
    dw = (d.w - s0.w) - (s1.w - s0.w)
    assert (np.abs(dw) <= TOL_G * max(np.abs(s1.w - s0.w).max(), 1e-9) + 1.2e-7 * np.abs(s1.w)).all()
    assert d.w0 - s0.w0 == pytest.approx(s1.w0 - s0.w0, rel=TOL_G, abs=1.2e-7 * abs(s1.w0) + 1e-9)
    # what the twin leaves untouched keeps every bit
    untouched = ~(tv[:, :, None] & np.ones_like(d.v, bool))
    assert np.array_equal(d.v[untouched], s0.v[untouched]) and np.array_equal(d.w[~tw], s0.w[~tw])
    assert (d.v[~untouched] != s0.v[~untouched]).mean() > 0.9          # ... and what it touches moved
    if ada:
        gtol = 2 * rowtol(s1.nv - s0.nv)[:, None, None] + 3e-7 * s1.nv
        assert (np.abs((d.nv - s0.nv) - (s1.nv - s0.nv)) <= gtol).all()
        assert (np.abs((d.nw - s0.nw) - (s1.nw - s0.nw)) <= 2 * TOL_G * max(np.abs(s1.nw - s0.nw).max(), 1e-12) + 3e-7 * s1.nw).all()
        assert d.n0 - s0.n0 == pytest.approx(s1.n0 - s0.n0, rel=2 * TOL_G, abs=3e-7 * s1.n0)
        assert np.array_equal(d.nv[untouched], s0.nv[untouched]) and np.array_equal(d.nw[~tw], s0.nw[~tw])


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("optimizer", ["sgd", "adagrad"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_step_vs_twin(fmhip, step_rows, shape, optimizer, loss):
    (F, k), used, (rows, y) = shape, SHAPES[shape], step_rows[shape]
    ada, linear = optimizer == "adagrad", shape != (3, 4)          # (the Kp = 4 shape is libffm's model: w0 and w never step)
    kw = dict(eta=0.05, reg0=0.01, regw=0.02, regv=0.03)
    hip = fmhip.HipFFM.run(loss=loss, optimizer=optimizer, adagrad_init=0.1, linear=linear, **kw)
    m = device_model(fmhip, start(11, STEP_N1, F, k), F, k, hip)
    ds = fmhip.FFMDataSet.from_rows(rows, y, batch_rows=600)
    for b, (lo, hi) in enumerate(((0, 600), (600, 601))):          # the batch of 600 rows, then the batch of one row
        s0 = device_state(m, ada)
        s1 = copy.deepcopy(s0)
        tv, tw = ref.step(s1, rows[lo:hi], y[lo:hi], loss=loss, optimizer=optimizer, linear=linear, **kw)
        unused = np.setdiff1d(np.arange(F), used)
        assert b == 1 or (tv[0, used].all() and tv[4].sum() == 2 and not tv[:, unused].any() and not tw[40])          # both kinds of (i, f)
        st = hip.step(m, ds, b)
        assert st["rows"] == hi - lo and st["steps"] == 1 and st["nonfinite"] == 0
        check_step(m, s0, s1, tv, tw, ada)
        assert linear or (m.w0 == s0.w0 and not tw.any())          # (check_step: w keeps every bit where tw is False)


def test_accumulators_round_trip(fmhip):
    m = device_model(fmhip, start(3, 6, 2, 5), 2, 5, fmhip.HipFFM.run(adagrad_init=0.5))
    n0, nw, nv = 0.25, f32(np.arange(6) / 7), f32(np.arange(60).reshape(6, 2, 5) / 61)
    m.set_adagrad_state(n0, nw, nv)
    got = m.adagrad_state()
    assert got[0] == n0 and np.array_equal(got[1], nw) and np.array_equal(got[2], nv)
    with pytest.raises(RuntimeError, match="finite and >= 0"):
        m.set_adagrad_state(n0, nw, -nv)


REFUSALS = [(dict(col=[1, 9]), {}, "step", b"feature id 9, above the model's num_attribute = 8"),
            (dict(field=[0, 3]), {}, "step", b"field id 3, outside the model's [0, 3)"),
            ({}, dict(y=None), "step", b"created without labels"), ({}, dict(y=None), "epoch", b"created without labels")]


@pytest.mark.parametrize("data,kw,call,msg", REFUSALS)
def test_pairing_refusals(fmhip, data, kw, call, msg):
    """A call that pairs a model with data it cannot hold: -1, the value named, nothing launched (the parameters keep every bit)."""
    from sparkfm_amd import _ffi
    L = _ffi.load()
    d = dict(dict(row_ptr=[0, 2], col=[1, 2], field=[0, 1], val=[1.0, 1.0], y=[1.0]), **data, **kw)
    ds = fmhip.FFMDataSet(d["row_ptr"], d["col"], d["field"], d["val"], d["y"])
    m = device_model(fmhip, start(1, 9, 3, 4), 3, 4, fmhip.HipFFM.run())
    before = m.get_params()
    rc = (L.fmhip_ffm_step(m.handle, ds.handle, 0, 0.1, 0.0, 0.0, 0.0, None) if call == "step" else
          L.fmhip_ffm_epoch(m.handle, ds.handle, 0.1, 0.0, 0.0, 0.0, None, None))
    assert rc == -1 and msg in L.fmhip_last_error()
    if "y" not in kw:
        assert L.fmhip_ffm_predict(m.handle, ds.handle, _ffi.ptr(np.zeros(1))) == -1 and msg in L.fmhip_last_error()
    assert all(np.array_equal(a, b) for a, b in zip(before, m.get_params()))


def test_epoch_is_deterministic_and_follows_the_order(fmhip, step_rows):
    (F, k), (rows, y) = (7, 5), [x[:301] for x in step_rows[(7, 5)]]
    kw = dict(eta=0.05, reg0=0.01, regw=0.02, regv=0.03)
    hip = fmhip.HipFFM.run(loss="logistic", optimizer="adagrad", adagrad_init=0.1, **kw)
    ds = fmhip.FFMDataSet.from_rows(rows, y, batch_rows=64)          # 4 batches of 64 and one of 45
    order, outs = [3, 0, 4, 2, 1], []
    for _ in range(2):
        s = start(12, STEP_N1, F, k, init=0.1)
        m = device_model(fmhip, s, F, k, hip)
        hip.learn(m, ds, order)
        assert hip.last_stats["rows"] == 301 and hip.last_stats["steps"] == 5
        outs.append(m.get_params() + m.adagrad_state())
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    ref.epoch(s, rows, y, 64, order=order, loss="logistic", optimizer="adagrad", **kw)
    s0 = start(12, STEP_N1, F, k)
    assert (np.abs((outs[0][2] - s0.v) - (s.v - s0.v)) <= rowtol(s.v - s0.v)[:, None, None] + 1.2e-7 * np.abs(s.v)).all()


def test_twenty_epochs_on_the_planted_task(fmhip):
    t = ref.planted()
    s, want_train, want_test = ref.run_planted(t)
    (xtr, ytr), (xte, yte) = t["train"], t["test"]
    hip = fmhip.HipFFM.run(loss="logistic", optimizer="adagrad", eta=ref.P_ETA, regv=ref.P_REGV, maxIteration=ref.P_EPOCHS, adagrad_init=1.0)
    m = device_model(fmhip, ref.planted_init(t, ref.P_FIELDS), ref.P_FIELDS, ref.P_K, hip)
    train = fmhip.FFMDataSet.from_rows(xtr, ytr, batch_rows=ref.P_BATCH)
    hip.fit(m, train)
    got_train, got_test = m.computeLogLoss(train), m.computeLogLoss(fmhip.FFMDataSet.from_rows(xte, yte))
    print("train %.8f (twin %.8f), test %.8f (twin %.8f)" % (got_train, want_train, got_test, want_test))
    assert got_train == pytest.approx(want_train, rel=1e-5) and got_test == pytest.approx(want_test, rel=1e-5)
