"""The BPR trainer's sampled softmax on the GPU (include/fmhip_softmax.h) against the fp64 twin of softmax_ref.py: steps at every
group width of the pre-pass (n_neg 1, 2, 3, 7 and 70 — above a wavefront) with and without the log-Q correction, n_neg = 1 against
logistic BPR, three-epoch trajectories in both redraw modes and under the best-of-C sampler, bit-identical reruns, the switch
turned off, the refusals, and a non-finite row."""
import ctypes as C

import numpy as np
import pytest

import bpr_proposal_ref as pref
import bpr_ref as bref
import softmax_ref as sref
import train_ref as ref
from test_gpu_adagrad import EPS, check_step as check_adagrad_step, get_state
from test_gpu_weights import check_step
from train_ref import rel, same

pytestmark = pytest.mark.gpu

REGS = (1e-3, 2e-3, 3e-3)
ERR_INVALID = -1             # FMHIP_ERR_INVALID
ETA = 0.05


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def L():
    from sparkfm_amd import _ffi
    return _ffi.load()


def params(fm):
    return fm.w0, fm.w.copy(), fm.v.copy()


def close(bpr, fm=None):
    bpr.close()
    bpr.contexts.unpersist()
    bpr.candidates.unpersist()
    if fm is not None:
        fm.close()


def problem(seed, k, n_neg, n_inter=150):
    """bpr_ref's problem at 30 contexts and 80 candidate rows."""
    return bref.make_problem(seed, k, n_ctx=30, M=80, n_inter=n_inter, n_neg=n_neg)


def weights_of(P):
    """A non-uniform proposal: one weight per candidate row, a factor of 30 between the lightest and the heaviest."""
    return np.exp(np.random.default_rng(P["seed"] + 7).uniform(0.0, np.log(30.0), P["M"]))


def twin_settings(optimizer):
    return ref.Rule("logistic", True, EPS if optimizer == "adagrad" else None), 0.1 if optimizer == "adagrad" else 0.0


# ---- 1. steps against the twin -----------------------------------------------------------------------------------------------------

# k -> Kp: 4 and 8 -> 32 (packed e), 33 -> 64 (packed); n_neg -> the pre-pass's group width: 1, 2, 4, 8, 64 (70: strode over)
@pytest.mark.parametrize("n_neg", [1, 2, 3, 7, 70])
@pytest.mark.parametrize("k", [4, 8, 33])
def test_steps_vs_twin(fmhip, k, n_neg):
    """Two batches of whole interactions, the second shorter; draws at t = 2 from a non-uniform weight array.  For SGD and AdaGrad,
    with and without logq: the step of batch 0 against the twin by the project's one-step check (test_gpu_weights.check_step /
    test_gpu_adagrad.check_step), then the step of batch 1 and rel-L2 1e-5 on v and w, softmax_probs() to 1e-5 absolute, the last
    step's statistics (rows = 2 * pairs, sum_e exactly 0, sse = 2 sum g^2 to rel 1e-5) and the scoring call.  At n_neg = 70 there
    are 40 interactions (5600 rows), else 150."""
    n_inter = 40 if n_neg == 70 else 150
    P = problem(1000 + 10 * k + n_neg, k, n_neg, n_inter)
    w = weights_of(P)
    table = pref.alias_table(w)
    neg = pref.draw(P, 2, table)[0]
    p = bref.layout(P, neg)
    n_pairs = len(neg)
    bp = n_neg * (n_inter // 2 + 3)
    r_cut = 2 * bp
    for optimizer in ("sgd", "adagrad"):
        for logq in (False, True):
            kw = dict(loss="softmax", logq=logq, negatives=w, optimizer=optimizer, eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2])
            if optimizer == "adagrad":
                kw.update(adagrad_eps=EPS, adagrad_init=0.1)
            bpr, fm = bref.build(fmhip, P, batch_pairs=bp, **kw)
            assert bpr.n_batches == 2 and bpr.n_pairs == n_pairs
            lq = sref.logq(w) if logq else None
            got_lq = bpr.logq
            assert (got_lq is None) if lq is None else np.array_equal(got_lq, lq)
            bpr.resample(2)
            assert np.array_equal(bpr.negatives(), neg)
            rule, init = twin_settings(optimizer)
            s0 = ref.State(P["w0"], P["w"], P["v"], init)
            s1 = s0.copy()
            e0, _, _ = sref.step(s1, p, 0, r_cut, n_neg, ETA, *REGS, rule, lq)
            st = bpr.step(fm, 0)
            if optimizer == "adagrad":
                check_adagrad_step(fm, s0, s1, 0.1, ETA)
            else:
                check_step(fm, s0, s1)
            assert st["rows"] == r_cut and st["sum_e"] == 0.0 and st["nonfinite"] == 0 and st["sse"] == pytest.approx((e0 * e0).sum(), rel=1e-5)
            s2 = s1.copy()
            e1, _, _ = sref.step(s2, p, r_cut, 2 * n_pairs, n_neg, ETA, *REGS, rule, lq)
            st = bpr.step(fm, 1)
            assert rel(fm.v, s2.v) <= 1e-5 and rel(fm.w, s2.w) <= 1e-5, (optimizer, logq, rel(fm.v, s2.v), rel(fm.w, s2.w))
            assert fm.w0 == pytest.approx(s2.w0, rel=1e-5, abs=1e-6)
            assert st["rows"] == 2 * n_pairs - r_cut and st["steps"] == 1 and st["sum_e"] == 0.0 and st["nonfinite"] == 0
            assert st["sse"] == pytest.approx((e1 * e1).sum(), rel=1e-5)
            pi = bpr.softmax_probs()
            assert pi.dtype == np.float32 and np.abs(pi - np.concatenate([-e0[0::2], -e1[0::2]])).max() <= 1e-5
            loss, top = sref.score(s2, p, n_neg, lq)
            assert bpr.computeSoftmaxLoss(fm) == pytest.approx(loss, rel=1e-5) and abs(bpr.computeTop1(fm) - top) <= 2 / n_inter
            close(bpr, fm)
    # the correction is not a no-op on this problem
    assert np.ptp(sref.logq(w)) > 3.0


def test_n_neg_one_is_logistic_bpr(fmhip):
    """With n_neg = 1, loss="softmax" trains to within rel 1e-5 of loss="logistic" from the same start (three epochs of two
    batches).  The bits may differ: the logistic pair rule forms sigma(-d) as z / (1 + z) or 1 / (1 + z) from z = exp(-|d|), the
    softmax as exp(a - mx) / (exp(-mx) + exp(a - mx)) — the same number through other roundings."""
    P = problem(1200, 8, 1)
    out = []
    for loss in ("softmax", "logistic"):
        bpr, fm = bref.build(fmhip, P, batch_pairs=80, loss=loss, eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2])
        for _ in range(3):
            bpr.learn(fm)
        out.append((params(fm), bpr.negatives(), bpr.last_stats))
        close(bpr, fm)
    (a, na, sa), (b, nb, sb) = out
    assert np.array_equal(na, nb)
    assert rel(a[2], b[2]) <= 1e-5 and rel(a[1], b[1]) <= 1e-5 and a[0] == pytest.approx(b[0], rel=1e-5, abs=1e-6)
    assert sa["sse"] == pytest.approx(sb["sse"], rel=1e-5) and sa["rows"] == sb["rows"] and sa["sum_e"] == sb["sum_e"] == 0.0
    assert np.abs(a[2] - P["v"]).max() > 1e-4


# ---- 2. trajectories ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_candidates", [1, 4])
@pytest.mark.parametrize("redraw", ["epoch", "batch"])
def test_three_epochs_vs_twin(fmhip, redraw, n_candidates):
    """Three epochs of two batches, n_neg = 3, the last batch short but of whole interactions (150 interactions: 80 and 70), under
    the popularity proposal with logq — in both redraw modes, with the uniform sampler and with the best of 4 candidates feeding
    the softmax: the kept negatives equal the twin's, rel-L2 1e-5 on v and w, computeSoftmaxLoss to rel 1e-5, computeTop1 within
    2 / interactions."""
    n_neg, k = 3, 8
    P = problem(1300, k, n_neg)
    w = pref.popularity(P)
    bpr, fm = bref.build(fmhip, P, batch_pairs=240, loss="softmax", logq=True, negatives="popularity", redraw=redraw, n_candidates=n_candidates,
                         eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2])
    assert bpr.n_batches == 2 and bpr.n_pairs == 450 and np.array_equal(bpr.proposal, w)
    for _ in range(3):
        bpr.learn(fm)
    lq = sref.logq(w)
    s, got = sref.epochs(ref.State(P["w0"], P["w"], P["v"]), P, 3, 240, ETA, *REGS, ref.Rule("logistic", True, None), lq=lq,
                         table=pref.alias_table(w), C=n_candidates, redraw=redraw)
    assert np.array_equal(bpr.negatives(), got["neg"])
    assert rel(fm.v, s.v) <= 1e-5 and rel(fm.w, s.w) <= 1e-5, (rel(fm.v, s.v), rel(fm.w, s.w))
    assert fm.w0 == pytest.approx(s.w0, rel=1e-5, abs=1e-6)
    assert np.abs(fm.v - P["v"]).max() > 1e-4
    st = bpr.last_stats
    assert st["rows"] == 900 and st["steps"] == 2 and st["sum_e"] == 0.0 and st["sse"] == pytest.approx(got["sse"], rel=1e-5)
    assert np.abs(bpr.softmax_probs() - got["pi"]).max() <= 1e-5
    loss, top = sref.score(s, bref.layout(P, got["neg"]), n_neg, lq)
    assert bpr.computeSoftmaxLoss(fm) == pytest.approx(loss, rel=1e-5) and abs(bpr.computeTop1(fm) - top) <= 2 / 150
    close(bpr, fm)


def test_bit_identical_run_to_run(fmhip):
    """Two fresh handles and models, same seed: the same bits of w0, w and v after two epochs (AdaGrad, n_neg = 7, three batches,
    the popularity proposal with logq), and the same probabilities."""
    P = problem(1400, 33, 7)
    runs = []
    for _ in range(2):
        bpr, fm = bref.build(fmhip, P, batch_pairs=7 * 60, loss="softmax", logq=True, negatives="popularity", optimizer="adagrad", eta=ETA,
                             reg0=REGS[0], regw=REGS[1], regv=REGS[2])
        assert bpr.n_batches == 3
        for _ in range(2):
            bpr.learn(fm)
        runs.append((params(fm), bpr.softmax_probs(), bpr.last_stats, get_state(fm)))
        close(bpr, fm)
    a, b = runs
    assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[0][1], b[0][1]) and np.array_equal(a[0][2], b[0][2])
    assert np.array_equal(a[1], b[1]) and a[2] == b[2] and same(a[3], b[3])
    assert np.abs(a[0][2] - P["v"]).max() > 1e-4


# ---- 3. the switch -----------------------------------------------------------------------------------------------------------------

def test_switch_off_is_the_parent_path(fmhip):
    """A loss="logistic" handle trains the same bits whether it is made before or after a softmax handle has lived and trained in
    the process; and a softmax handle whose switch is turned off (fmhip_softmax_set(h, 0, 0)), with the model's loss set by hand,
    trains those bits too."""
    from sparkfm_amd import _ffi
    P = problem(1500, 8, 3)
    kw = dict(batch_pairs=240, eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2])

    def run(loss, switch_off=False):
        bpr, fm = bref.build(fmhip, P, loss=loss, **kw)
        if switch_off:
            _ffi.check(L().fmhip_softmax_set(bpr.handle, 0, 0))
            _ffi.check(L().fmhip_model_set_loss(fm.handle, _ffi.LOSS_LOGISTIC))
        for _ in range(2):
            bpr.learn(fm)
        out = params(fm), bpr.last_stats
        close(bpr, fm)
        return out

    before = run("logistic")
    softmax = run("softmax")
    after = run("logistic")
    off = run("softmax", switch_off=True)
    for other in (after, off):
        assert np.array_equal(before[0][0], other[0][0]) and np.array_equal(before[0][1], other[0][1]) and np.array_equal(before[0][2], other[0][2])
        assert before[1] == other[1]
    assert not np.array_equal(before[0][2], softmax[0][2])      # (n_neg = 3: the softmax is another rule)


def test_refusals_name_the_item(fmhip):
    from sparkfm_amd import _ffi
    P = problem(1600, 4, 3)
    err = lambda: L().fmhip_last_error().decode()      # noqa: E731
    en, lg = C.c_int(), C.c_int()
    # WARP, then the softmax
    bpr, fm = bref.build(fmhip, P, batch_pairs=240, sampler="warp", n_candidates=4)
    h = bpr.handle
    assert L().fmhip_softmax_set(h, 1, 0) == ERR_INVALID and "WARP is on" in err() and "fmhip_softmax_set" in err()
    _ffi.check(L().fmhip_softmax_get(h, C.byref(en), C.byref(lg)))
    assert (en.value, lg.value) == (0, 0)
    _ffi.check(L().fmhip_softmax_set(h, 0, 1))                   # (turning it off is never refused)
    close(bpr, fm)
    # the softmax, then WARP
    bpr, fm = bref.build(fmhip, P, batch_pairs=240, loss="softmax")
    h = bpr.handle
    _ffi.check(L().fmhip_softmax_get(h, C.byref(en), C.byref(lg)))
    assert (en.value, lg.value) == (1, 0)
    assert L().fmhip_warp_set(h, 1, 1.0) == ERR_INVALID and "the softmax switch is on" in err() and "fmhip_warp_set" in err()
    mg = C.c_double()
    _ffi.check(L().fmhip_warp_get(h, C.byref(en), C.byref(mg)))
    assert en.value == 0
    # softmax_probs() before any step, and before every batch has had one
    with pytest.raises(_ffi.FmhipError, match="no softmax probabilities stand"):
        bpr.softmax_probs()
    bpr.step(fm, 0)
    with pytest.raises(_ffi.FmhipError, match="no softmax probabilities stand"):
        bpr.softmax_probs()
    bpr.step(fm, 1)
    assert bpr.softmax_probs().shape == (450,)
    # the uniform proposal: no table to read
    one = np.zeros(P["M"], np.float32)
    assert L().fmhip_softmax_logq(h, _ffi.ptr(one)) == ERR_INVALID and "not in force" in err()
    close(bpr, fm)
    # a batch that splits an interaction: the C call names both numbers and leaves the handle as it was; so does Python
    bpr, fm = bref.build(fmhip, P, batch_pairs=100)
    h = bpr.handle
    assert L().fmhip_softmax_set(h, 1, 0) == ERR_INVALID and "batch_pairs = 100" in err() and "n_neg = 3" in err()
    _ffi.check(L().fmhip_softmax_get(h, C.byref(en), C.byref(lg)))
    assert (en.value, lg.value) == (0, 0)
    loss = C.c_double()
    assert L().fmhip_softmax_loss(fm.handle, h, C.byref(loss), None, None) == ERR_INVALID and "batch_pairs = 100" in err()
    close(bpr, fm)
    with pytest.raises(ValueError, match="batch_pairs = 100 is no multiple of n_neg = 3"):
        bref.build(fmhip, P, batch_pairs=100, loss="softmax")


def test_the_table_follows_the_proposal(fmhip):
    """bpr.logq is the twin's table bit for bit, is rebuilt by set_proposal, and is gone under the uniform proposal — whose steps
    then have the bits of logq=False."""
    P = problem(1700, 8, 3)
    w = weights_of(P)
    bpr, fm = bref.build(fmhip, P, loss="softmax", logq=True, negatives=w, eta=ETA)
    assert np.array_equal(bpr.logq, sref.logq(w))
    bpr.set_proposal(w[::-1].copy())
    assert np.array_equal(bpr.logq, sref.logq(w[::-1]))
    bpr.set_proposal(None)
    assert bpr.logq is None
    bpr.learn(fm)
    bpr2, fm2 = bref.build(fmhip, P, loss="softmax", logq=False, eta=ETA)
    bpr2.learn(fm2)
    assert np.array_equal(fm.v, fm2.v) and np.array_equal(fm.w, fm2.w) and np.array_equal(bpr.softmax_probs(), bpr2.softmax_probs())
    close(bpr, fm)
    close(bpr2, fm2)


# ---- 4. a non-finite row -----------------------------------------------------------------------------------------------------------

def test_a_nan_row_zeroes_its_interactions_only(fmhip):
    """Feature f of the candidates block gets a NaN row of v.  Every interaction with an item that holds f — as its positive or as
    one of its negatives — has g = 0 for all its pairs and adds nothing to any gradient; its rows count as non-finite.  The other
    interactions train as in the twin: w everywhere and every other row of v to rel 1e-5, the probabilities to 1e-5."""
    n_neg, k = 3, 8
    P = problem(1800, k, n_neg)
    items = P["items"]
    f = int(items["col"][items["row_ptr"][11]])            # the first feature of item row 11
    P["v"] = P["v"].copy()
    P["v"][:, f] = np.nan
    bpr, fm = bref.build(fmhip, P, loss="softmax", eta=ETA, reg0=REGS[0], regw=REGS[1], regv=REGS[2])
    bpr.resample(1)
    neg = bref.draw(P, 1)[0]
    p = bref.layout(P, neg)
    s = ref.State(P["w0"], P["w"], P["v"])
    e, _, _ = sref.step(s, p, 0, 2 * len(neg), n_neg, ETA, *REGS, ref.Rule("logistic", True, None))
    st = bpr.step(fm, 0)
    pi = bpr.softmax_probs()
    holds = np.array([f in items["col"][items["row_ptr"][i]:items["row_ptr"][i + 1]] for i in range(P["M"])])
    mi = p["maps"][1]
    bad_rows = holds[mi]
    bad_inter = bad_rows.reshape(-1, 2 * n_neg).any(axis=1)
    assert 0 < bad_inter.sum() < len(bad_inter)
    assert (pi.reshape(-1, n_neg)[bad_inter] == 0.0).all() and (pi.reshape(-1, n_neg)[~bad_inter] > 0.0).all()
    assert np.abs(pi - (-e[0::2])).max() <= 1e-5
    assert st["nonfinite"] == int(bad_rows.sum()) and st["sum_e"] == 0.0 and st["sse"] == pytest.approx((e * e).sum(), rel=1e-5)
    keep = np.arange(P["n1"]) != f
    gv, sv = fm.v, s.v
    assert np.isfinite(gv[:, keep]).all() and np.isfinite(sv[:, keep]).all() and np.isfinite(fm.w).all()
    assert rel(gv[:, keep], sv[:, keep]) <= 1e-5 and rel(fm.w, s.w) <= 1e-5
    assert np.isnan(gv[:, f]).all()
    close(bpr, fm)


# ---- 5. include/sparkfm.hpp --------------------------------------------------------------------------------------------------------

def test_cpp_softmax_matches_python(fmhip, tmp_path):
    """tests/cpp_softmax.cpp (include/sparkfm.hpp's HipBPR with loss = kSoftmax, kPopularity and logq) against the Python mirror over
    the integer formulas of tests/cpp_bpr.cpp: with the C++ side's weights handed to the mirror, the log-Q table, the draw and every
    parameter after two epochs, the probabilities, the loss and top1, hex floats equal; the program checks its refusals itself."""
    import os
    import subprocess
    from sparkfm_amd import _build
    from test_gpu_bpr import cpp_problem
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_softmax")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_softmax.cpp"), "-L" + _build.LIBDIR, "-lfmhip",
                           "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = {ln.split()[0]: [float.fromhex(t) for t in ln.split()[1:]] for ln in out.stdout.decode().splitlines()}
    c = cpp_problem()
    mk = lambda b: fmhip.DataSet(b["row_ptr"], b["col"], b["val"], np.zeros(len(b["row_ptr"]) - 1), batch_rows=0)      # noqa: E731
    w = np.array(got["weights"])
    bpr = fmhip.HipBPR.run(mk(c["users"]), mk(c["items"]), c["positives"], n_neg=3, batch_pairs=99, seed=5, shuffle=False, eta=0.05, regw=1e-4,
                           regv=1e-4, loss="softmax", logq=True, negatives=w)
    fm = fmhip.FMModel(c["n1"] - 1, c["k"])
    fm.w0, fm.w, fm.v = c["w0"], c["w"], c["v"]
    assert bpr.n_batches == 4 and bpr.n_pairs % 99 == 39
    assert got["logq"] == bpr.logq.tolist() == sref.logq(w).tolist() and len(set(got["logq"])) > 3
    bpr.learn(fm)
    bpr.learn(fm)
    assert got["neg"] == bpr.negatives().tolist()
    assert got["w0"] == [fm.w0] and got["w"] == fm.w.tolist() and got["v"] == fm.v.T.ravel().tolist()
    assert got["probs"] == bpr.softmax_probs().tolist()
    assert got["loss"] == [bpr.computeSoftmaxLoss(fm)] and got["top1"] == [bpr.computeTop1(fm)]
    st = bpr.last_stats
    assert got["stats"] == [st["rows"], st["sum_e"], st["sse"]] and st["sum_e"] == 0.0
    close(bpr, fm)
