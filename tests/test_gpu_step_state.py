"""What a mini-batch step hands from one of its pieces to the next (StepState, sparkfm_amd/csrc/fmhip_internal.h; DESIGN.md "The
step's state"), pinned from outside through the C ABI: who owns the packed gradient across a touched-rows step, what a refused
fmhip_step_backward leaves behind, a rank that runs out of rows in each of the four exchange modes, and two models sharing one
dataset between the pieces of a split step.

One small shape: 600 Zipf rows in 3 batches of 200, 300 features, 1 to 12 entries per row, the dense hot block on; k = 8
(Kp = 32) and k = 40 (Kp = 64, the widest the pipelined exchange takes); cuts at the fractions (0.3, 0.6) of the stored
nonzeros, so the interval backward, ranges that straddle a cut and the update of slices as they arrive all run."""
import ctypes as C

import numpy as np
import pytest

import oracle
import dp_cases

pytestmark = pytest.mark.gpu

ROWS, BATCH, N1 = 600, 200, 300
FRACTIONS = (0.3, 0.6)
ETA, REG0, REGW, REGV = 0.05, 0.0, 1e-3, 1e-3
KS = [8, 40]


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


@pytest.fixture(scope="module")
def data():
    from sparkfm_amd import synth
    d = synth.make_zipf(2026, ROWS, N1, 1, 12, zipf_s=1.05)
    return dict(row_ptr=d["row_ptr"], col=d["col"], val=d["val"].astype(np.float64), y=d["y"].astype(np.float64))


def start(k):
    from sparkfm_amd import synth
    _, _, v = synth.init_params(31 + k, N1, k, stdev=0.05)
    return 0.05, np.random.default_rng(32 + k).normal(0, 0.05, N1), v


def dataset(fmhip, data):
    ds = fmhip.DataSet(data["row_ptr"], data["col"], data["val"], data["y"], batch_rows=BATCH).cache()
    assert ds.layout()["hot_pages"] > 0 and ds.n_batches == 3          # hot_pending is live in every step below
    return ds


def model(fmhip, k, stream=None):
    fm = fmhip.FMModel(N1 - 1, k, stream=stream)
    fm.w0, fm.w, fm.v = start(k)
    return fm


def feature_cuts(data):
    """The feature ids at or above which the shares FRACTIONS of the stored nonzeros lie (what fmhip_dp_plan picks), ascending."""
    cnt = np.bincount(data["col"], minlength=N1)
    above = np.cumsum(cnt[::-1])[::-1]                                  # above[c] = nonzeros of the features >= c
    cuts = sorted(int(np.argmax(above <= f * cnt.sum())) for f in FRACTIONS)
    assert 0 < cuts[0] < cuts[1] < N1
    return cuts


def torch_stream():
    from sparkfm_amd.distributed import torch_stream_handle
    return torch_stream_handle(0)


# ---- 1. a gradient pending in the packed buffer survives a touched-rows step -------------------------------------------------

def pending_twin(data, k):
    """fp64: the gradient of batch 0 at theta_0, the step of batch 1 (theta_0 -> theta_1), then the batch-0 gradient applied at
    theta_1.  The packed gradient holds a V row's gradient as the pair (G_V, G_b) — gv = G_V - v * G_b, G_b[i] = sum_r e_r x_ri^2
    (fmhip_batch_grad reads it back so) — and the update forms it with the v it updates, so "applied at theta_1" is
    (G_V0 - v_1 G_b0) / |B| + regv v_1.  Also returned: the same with gv frozen at theta_0, for the record."""
    w0, w, v = start(k)
    rp, col, val, y = data["row_ptr"], data["col"], data["val"], data["y"]
    gv0, gw0, g00, _, e0 = oracle.batch_grad(w0, w, v, 0, BATCH, rp, col, val, y)
    nz = slice(int(rp[0]), int(rp[BATCH]))
    row_of = np.repeat(np.arange(BATCH), np.diff(rp[:BATCH + 1]))
    gb0 = np.bincount(col[nz], weights=np.asarray(e0)[row_of] * val[nz] ** 2, minlength=N1)
    GV0 = np.asarray(gv0) + v * gb0[None, :]
    w0_1, w_1, v_1, _ = oracle.sgd_step(w0, w, v, BATCH, 2 * BATCH, rp, col, val, y, ETA, REG0, REGW, REGV)
    w0_2 = w0_1 - ETA * (g00 / BATCH + REG0 * w0_1)
    w_2 = w_1 - ETA * (np.asarray(gw0) / BATCH + REGW * w_1)
    v_2 = v_1 - ETA * ((GV0 - v_1 * gb0[None, :]) / BATCH + REGV * v_1)
    v_2_frozen = v_1 - ETA * (np.asarray(gv0) / BATCH + REGV * v_1)
    return (w0_2, w_2, v_2), v_2_frozen, (w0_1, w_1, v_1)


@pytest.mark.parametrize("k", KS)
def test_pending_gradient_survives_a_touched_rows_step(fmhip, data, k):
    """fmhip_step_compute(batch 0), one touched-rows data-parallel step of batch 1 (world 1, thread-staged transport), then
    fmhip_step_apply: the touched-rows step writes its gradient rows into its compact buffer and neither cleans nor dirties the
    packed gradient, so batch 0's gradient is still there and the apply applies it.  Against the fp64 twin of that sequence
    (pending_twin) at test_gpu_parity.py's tolerance for parameters after a few steps: rel-L2 1e-4 on v and w, w0 to rel 1e-4
    + 1e-6 (test_sgd_epochs_track_the_oracle).
    The gradient's head belongs to it too: sum e is w0's gradient and the row count what the update divides by.  The touched-rows
    step used to copy ITS sums over them for fmhip_step_stats, and w0 then took batch 1's sum e — measured before that was mended,
    with v and w at 5e-8 of the twin: w0 = 0.0568571 against the twin's 0.0590907 at k = 8, 0.0542096 against 0.0562718 at k = 40.
    With a gradient pending the step now leaves the head alone (fmhip_step_stats then still reports the pending gradient's sums)."""
    from sparkfm_amd import _ffi
    from sparkfm_amd.distributed import HipDataParallelSGD, ThreadStagedComm, run_thread_ranks
    L = _ffi.load()

    def rank(r, group):
        ds, fm = dataset(fmhip, data), model(fmhip, k)
        comm = ThreadStagedComm(fm, r, group)
        dp = HipDataParallelSGD(comm, eta=ETA, reg0=REG0, regw=REGW, regv=REGV, exchange="touched", upper_fractions=FRACTIONS)
        dp.plan(fm, ds)
        assert len(dp.cuts) == 2
        _ffi.check(L.fmhip_step_compute(fm.handle, ds.handle, 0))
        dp.step_at(fm, ds, 1)
        _ffi.check(L.fmhip_step_apply(fm.handle, ETA, REG0, REGW, REGV))
        fm._device_updated()
        out = fm.w0, fm.w.copy(), fm.v.copy()
        group.barrier()
        comm.close()
        ds.unpersist()
        fm.close(discard=True)
        return out

    w0, w, v = run_thread_ranks(1, rank)[0]
    (t0, tw, tv), tv_frozen, (s0, sw, sv) = pending_twin(data, k)
    ev, ew = dp_cases.rel(v, tv), dp_cases.rel(w, tw)
    print("k=%d: rel-L2 v %.3g w %.3g, w0 %.9g (twin %.9g); v against gv frozen at theta_0 %.3g; against theta_1 (nothing applied) v %.3g w %.3g"
          % (k, ev, ew, w0, t0, dp_cases.rel(v, tv_frozen), dp_cases.rel(v, sv), dp_cases.rel(w, sw)))
    # the twin alone: leaving the pending gradient out moves v and w by more than three times what the assertions below allow
    assert dp_cases.rel(tv, sv) > 3e-4 and dp_cases.rel(tw, sw) > 3e-4 and abs(t0 - s0) > 3 * (1e-4 * abs(t0) + 1e-6)
    assert ev <= 1e-4 and ew <= 1e-4
    assert w0 == pytest.approx(t0, rel=1e-4, abs=1e-6)


# ---- 2. a refused fmhip_step_backward leaves the step usable -----------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_a_refused_interval_leaves_the_step_usable(fmhip, data, k):
    """After the forward a wrongly ordered interval is refused; the right intervals then run to completion and the packed
    gradient is fmhip_step_compute's bit for bit — descending, and ascending (there also a wrong interval in mid-sequence).
    After the last interval one more call is refused: the window is closed."""
    import torch
    from sparkfm_amd import _ffi
    from sparkfm_amd.distributed import HipEngine
    L = _ffi.load()
    ds, fm = dataset(fmhip, data), model(fmhip, k, stream=torch_stream())
    eng = HipEngine(fm, ds)
    c1, c2 = feature_cuts(data)

    def clean():
        torch.cuda.synchronize()
        eng.grad.zero_()
        torch.cuda.synchronize()
        _ffi.check(L.fmhip_grad_bind(fm.handle, C.c_void_p(eng.grad.data_ptr())))      # marks the zeroed buffer clean

    def refused(lo, hi, finish, text):
        assert L.fmhip_step_backward(fm.handle, ds.handle, 0, lo, hi, finish) == -1
        assert L.fmhip_last_error() == text, L.fmhip_last_error()

    eng.compute(0)
    torch.cuda.synchronize()
    want = eng.grad.clone()
    clean()
    down = b"feature intervals must tile [0, n+1) in descending order (expected hi = %d, got %d), or start at feature 0 and ascend"
    up = b"feature intervals must tile [0, n+1) in ascending order (expected lo = %d, got %d)"
    for ascending in (False, True):
        eng.forward(0)
        refused(c1, c2, 0, down % (N1, c2))                            # neither ends at n+1 nor starts at 0
        refused(c1, N1, 1, b"finish = 1 belongs to the interval that starts at feature 0")
        if ascending:
            eng.backward(0, 0, c1, finish=True)
            refused(c2, N1, 0, up % (c1, c2))
            refused(0, c1, 0, up % (c1, 0))
            eng.backward(0, c1, c2, finish=False)
            eng.backward(0, c2, N1, finish=False)
        else:
            eng.backward(0, c2, N1, finish=False)
            refused(0, c1, 1, down % (c2, c1))
            refused(c2, N1, 0, down % (c2, N1))
            eng.backward(0, c1, c2, finish=False)
            eng.backward(0, 0, c1, finish=True)
        refused(0, N1, 1, b"fmhip_step_backward without fmhip_step_forward")
        torch.cuda.synchronize()
        assert torch.equal(eng.grad, want), ascending
        clean()
    eng.close()
    ds.unpersist()
    fm.close()


# ---- 3. a rank that runs out of rows, in every exchange mode -----------------------------------------------------------------

@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("exchange", ["dense", "touched", "sharded", "pipelined"])
def test_a_rank_out_of_rows_in_every_exchange_mode(fmhip, exchange, k):
    """World 2 as thread ranks on one GPU: rank 0 holds 3 batches, rank 1 one, so rank 1 contributes zeros at the positions 1 and
    2 of the epoch — after a step of its own, with its gradient buffer as that step left it.  One epoch against the fp64 oracle
    over the global batches with dp_cases.check and its tolerance (1e-5); the replicas bit-identical, the same collectives on
    both ranks.  (test_gpu_world8.py has ranks out of rows among eight, at k = 32 and other cuts; not this shape.)"""
    cfg = dict(seed=2026, rows=[ROWS, BATCH], n1_data=N1, n1=N1, k=k, lo=1, hi=12, batch_rows=BATCH, exchange=exchange, fractions=list(FRACTIONS),
               epochs=1, eta=ETA, regw=REGW, regv=REGV, shuffle_seed=None)
    for r in (0, 1):
        ds = fmhip.DataSet.from_arrays(dp_cases.shard(cfg, r), batch_rows=BATCH).cache()
        # (rank 0's steps form a hot block; a dataset of one batch, rank 1's, gets none by the library's default)
        assert (ds.layout()["hot_pages"] > 0) == (r == 0) and ds.n_batches == (3, 1)[r]
        ds.unpersist()
    res = dp_cases.run_threads(cfg)
    assert len(res[0]["cuts"]) == 2 and res[0]["steps"] == 3 and res[0]["rows"] == BATCH       # the last global batch is rank 0's alone
    ev, ew = dp_cases.check(cfg, res)
    print("%s k=%d: rel-L2 v %.3g w %.3g" % (exchange, k, ev, ew))


# ---- 4. another model uses the dataset between the pieces of a split step ----------------------------------------------------

@pytest.mark.parametrize("k", KS)
def test_another_model_steps_on_the_dataset_between_forward_and_backward(fmhip, data, k):
    """Model A runs its forward; model B runs a whole step on the same dataset; A's backward — over the intervals, from the top
    down — then gives the bits it gives without B: what a step carries between its pieces is the model's, not the dataset's."""
    import torch
    from sparkfm_amd import _ffi
    from sparkfm_amd.distributed import HipEngine
    L = _ffi.load()
    ds = dataset(fmhip, data)
    fa, fb = model(fmhip, k, stream=torch_stream()), model(fmhip, k + 1)
    eng = HipEngine(fa, ds)
    c1, c2 = feature_cuts(data)
    grads = []
    for with_b in (False, True):
        eng.forward(0)
        if with_b:
            fmhip.HipSGD(eta=ETA, reg0=REG0, regw=REGW, regv=REGV).step(fb, ds, 1)
            _ffi.check(L.fmhip_synchronize(fb.handle))
        for lo, hi in ((c2, N1), (c1, c2), (0, c1)):
            eng.backward(0, lo, hi, finish=(lo == 0))
        torch.cuda.synchronize()
        grads.append(eng.grad.clone())
        eng.grad.zero_()
        torch.cuda.synchronize()
        _ffi.check(L.fmhip_grad_bind(fa.handle, C.c_void_p(eng.grad.data_ptr())))
    assert float(grads[0][32:].abs().max()) > 0 and torch.equal(grads[0], grads[1])
    assert not np.array_equal(fb.v, start(k + 1)[2].astype(np.float32))               # B did step
    eng.close()
    ds.unpersist()
    fa.close()
    fb.close()
