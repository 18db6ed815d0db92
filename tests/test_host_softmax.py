"""The BPR trainer's sampled softmax, host surface (no GPU): the header against the binding and the exported symbols, the refusals
that need no device, the Python keywords, the fp64 twin's rule (softmax_ref.py) against central finite differences of its own loss,
the twin at n_neg = 1 against bpr_ref's logistic epochs, the log-Q table of fmhip_host.cpp (bpr_log_proposal) as a stand-alone
program under AddressSanitizer and UBSan, and the twin's held-out NDCG on the harder planted task."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import bpr_adaptive_ref as aref
import bpr_proposal_ref as pref
import bpr_ref as bref
import softmax_ref as sref
import train_ref as ref
from train_ref import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOFTMAX_NAMES = {"fmhip_softmax_" + n for n in ("set", "get", "loss", "probs", "logq")}


def declared_in(header):
    hdr = open(os.path.join(ROOT, "include", header)).read()
    return set(re.findall(r"\b(fmhip_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))


# ---- symbols and keywords ----------------------------------------------------------------------------------------------------------

def test_header_matches_the_binding_and_the_library():
    from sparkfm_amd import _build, _ffi
    assert declared_in("fmhip_softmax.h") == set(_ffi.SYMBOLS_SOFTMAX) == SOFTMAX_NAMES
    L = _ffi.load()
    for name in _ffi.SYMBOLS_SOFTMAX:
        assert hasattr(L, name) and getattr(L, name).argtypes is not None and getattr(L, name).restype is C.c_int, name
    out = subprocess.run(["nm", "-D", "--defined-only", _build.LIB], stdout=subprocess.PIPE, check=True).stdout.decode()
    assert set(re.findall(r"\bT (fmhip_softmax_[a-z0-9_]+)", out)) == SOFTMAX_NAMES
    assert os.path.join("..", "..", "include", "fmhip_softmax.h") in _build.HIP_DEPS and "fm_softmax.hip" in _build.HIP_SOURCES
    # the softmax is the trainer's own rule: the model's losses do not learn it
    with pytest.raises(ValueError):
        _ffi.loss_code("softmax")
    assert sorted(_ffi.LOSSES) == ["logistic", "squared"]


def test_c_calls_refuse_null_handles_without_a_device():
    from sparkfm_amd import _ffi
    L = _ffi.load()
    en, lg = C.c_int(-5), C.c_int(-5)
    loss = C.c_double(-5.0)
    one = np.zeros(1, np.float32)
    assert L.fmhip_softmax_set(None, 1, 0) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error()
    assert L.fmhip_softmax_get(None, C.byref(en), C.byref(lg)) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error()
    assert (en.value, lg.value) == (-5, -5)
    assert L.fmhip_softmax_loss(None, None, C.byref(loss), None, None) == -1 and b"NULL" in L.fmhip_last_error()
    assert loss.value == -5.0
    assert L.fmhip_softmax_probs(None, _ffi.ptr(one)) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error()
    assert L.fmhip_softmax_logq(None, _ffi.ptr(one)) == -1 and b"the BPR trainer is NULL" in L.fmhip_last_error()


def small_blocks():
    from sparkfm_amd import DataSet
    users = DataSet.from_rows([(0.0, ([0], [1.0])), (0.0, ([1], [1.0])), (0.0, ([], []))], batch_rows=0)
    items = DataSet.from_rows([(0.0, ([3 + j], [1.0])) for j in range(4)], batch_rows=0)
    return users, items, [[2, 0], [3], [1]]


def test_python_validates_the_keywords_at_construction():
    from sparkfm_amd import HipBPR
    users, items, pos = small_blocks()
    plain = HipBPR.run(users, items, pos)
    assert (plain.softmax, plain.logq, plain.loss) == (False, None, "logistic")
    sm = HipBPR.run(users, items, pos, loss="softmax", n_neg=3, logq=True)
    assert (sm.softmax, sm.loss, sm.n_neg, sm.n_pairs) == (True, "softmax", 3, 12)
    assert sm.logq is None                                  # (a uniform proposal: logq is ignored, before any device call)
    assert HipBPR.run(users, items, pos, loss="softmax", n_neg=3, batch_pairs=6).batch_pairs == 6
    assert HipBPR.run(users, items, pos, loss="softmax", n_neg=3, batch_pairs=100).batch_pairs == 12      # (one batch)
    with pytest.raises(ValueError, match=r"batch_pairs = 4 is no multiple of n_neg = 3"):
        HipBPR.run(users, items, pos, loss="softmax", n_neg=3, batch_pairs=4)
    assert HipBPR.run(users, items, pos, n_neg=3, batch_pairs=4).batch_pairs == 4      # (independent pairs may be cut anywhere)
    with pytest.raises(ValueError, match="sampler='warp'.*loss='softmax'"):
        HipBPR.run(users, items, pos, loss="softmax", sampler="warp")
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="logq must be True or False"):
            HipBPR.run(users, items, pos, loss="softmax", logq=bad)
    with pytest.raises(ValueError, match="belongs to loss='softmax'"):
        plain.softmax_probs()
    with pytest.raises(AttributeError):
        sm.softmax = False


# ---- the rule ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_lq", [False, True])
@pytest.mark.parametrize("n", [1, 3, 7])
def test_residuals_are_the_gradient_of_the_loss(n, with_lq):
    """e_2p = g_p, e_2p+1 = -g_p of softmax_ref.rule equal the central finite differences of sum_j loss_j with respect to each of the
    2 * pairs predictions, to 1e-6 relative (||fd - e|| / ||e||).  h = 1e-5: the difference's truncation error is h^2 |f'''| / 6 <
    2e-11 and its rounding error eps |loss| / h < 1e-10 per entry, against entries of order 1 / (n + 1)."""
    rng = np.random.default_rng(100 + 10 * n + with_lq)
    inter = 9
    yh = rng.normal(0, 1.5, 2 * n * inter)
    corr = rng.normal(0, 1.0, n * inter) if with_lq else None
    total = lambda y: float(sref.rule(y[0::2] - y[1::2], n, corr)[1].sum())      # noqa: E731
    g, loss, _ = sref.rule(yh[0::2] - yh[1::2], n, corr)
    e = np.empty(len(yh))
    e[0::2], e[1::2] = g, -g
    h = 1e-5
    fd = np.empty(len(yh))
    for r in range(len(yh)):
        up, dn = yh.copy(), yh.copy()
        up[r] += h
        dn[r] -= h
        fd[r] = (total(up) - total(dn)) / (2 * h)
    assert rel(fd, e) < 1e-6
    # the probabilities of an interaction and the positive's add to one; the loss is -log of the positive's
    pi = -g.reshape(inter, n)
    assert np.allclose(np.exp(-loss) + pi.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    if n == 1 and not with_lq:
        d = yh[0::2] - yh[1::2]
        assert np.allclose(g, ref.pair_g(d, np.ones_like(d), "logistic"), rtol=0, atol=1e-15)
        assert np.allclose(loss, ref.pair_loss(d, np.ones_like(d), "logistic"), rtol=0, atol=1e-15)


def test_rule_on_a_hand_table():
    ln = np.log
    g, loss, top = sref.rule([0.0, 0.0, 0.0], 3)
    assert np.allclose(g, -0.25) and np.allclose(loss, ln(4.0)) and top.tolist() == [False]      # (a tie is not on top)
    g, loss, top = sref.rule([1.0, 2.0, 800.0, -800.0], 2)
    z = 1.0 + np.exp(-1.0) + np.exp(-2.0)
    assert np.allclose(g[:2], [-np.exp(-1.0) / z, -np.exp(-2.0) / z]) and np.allclose(loss[0], ln(z)) and top.tolist() == [True, False]
    assert np.allclose(g[2:], [0.0, -1.0]) and np.allclose(loss[1], 800.0)                        # (no overflow: mx carries it)
    # the correction moves the logits: a negative twice as likely under the proposal counts half
    g, loss, _ = sref.rule([0.0], 1, [ln(2.0)])
    assert np.allclose(g, -1.0 / 3.0) and np.allclose(loss, ln(1.5))
    # a non-finite margin zeroes its whole interaction and nothing else
    g, loss, top = sref.rule([np.nan, 1.0, 0.0, 0.0, np.inf, 0.0], 2)
    assert g[:2].tolist() == [0.0, 0.0] and loss[0] == 0.0 and not top[0]
    assert np.allclose(g[2:4], -1.0 / 3.0) and np.allclose(loss[1], ln(3.0))
    assert g[4:].tolist() == [0.0, 0.0] and loss[2] == 0.0 and not top[2]


@pytest.mark.parametrize("eps", [None, 1e-10])
def test_n_neg_one_is_the_logistic_twin(eps):
    """With n_neg = 1 and no correction the twin's epochs equal bpr_ref's logistic epochs to 1e-12 (SGD and AdaGrad; three epochs
    of two batches)."""
    P = bref.make_problem(61, 4, n_ctx=12, M=30, n_inter=90, n_neg=1)
    rule = ref.Rule("logistic", True, eps)
    s0 = ref.State(P["w0"], P["w"], P["v"], 0.1)
    a, got = sref.epochs(s0.copy(), P, 3, 60, 0.05, 1e-3, 2e-3, 3e-3, rule)
    b, p = bref.epochs(s0.copy(), P, 3, 60, 0.05, 1e-3, 2e-3, 3e-3, rule)
    assert np.array_equal(got["neg"], p["maps"][1][1::2])
    assert abs(a.w0 - b.w0) <= 1e-12 and rel(a.w, b.w) <= 1e-12 and rel(a.v, b.v) <= 1e-12
    assert rel(a.v, s0.v) > 1e-4                     # (it did train)


# ---- the log-Q table ---------------------------------------------------------------------------------------------------------------

def weight_sets():
    rng = np.random.default_rng(23)
    P = bref.make_problem(30, 4)
    return [pref.popularity(P), np.ones(7), np.array([1.0]), rng.random(120) + 1e-3, rng.lognormal(0, 3, 401),
            np.array([1e-300, 1.0, 1e300]), np.array([5e-324, 1e308, 1e308 / 3]), (np.arange(1000) + 1.0) ** 0.75]


def test_logq_is_the_log_of_the_normalised_weights():
    for w in weight_sets():
        lq = sref.logq(w)
        assert lq.dtype == np.float32 and lq.shape == w.shape and np.isfinite(lq).all() and (lq <= 0).all()
        if w.min() / w.sum() > 0:                    # (where no quotient underflows the formula is the plain one)
            assert np.array_equal(lq, np.log(w / w.sum()).astype(np.float32))
        else:
            assert np.allclose(lq, np.log(w) - np.log(w.sum()), rtol=1e-6)
    assert np.array_equal(sref.logq(np.ones(4)), np.full(4, np.log(0.25), np.float32))


def vectors(path):
    lines = []
    for w in weight_sets():
        lq = sref.logq(w)                             # (== np.log(w / w.sum()).astype(float32) where no quotient underflows: above)
        lines.append("L %d %s %s" % (len(w), " ".join("%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0] for x in w),
                                    " ".join("%08x" % struct.unpack("<I", struct.pack("<f", float(x)))[0] for x in lq)))
    open(path, "w").write("\n".join(lines) + "\n")
    return len(lines), lines


def test_host_logq_under_the_sanitizers(tmp_path):
    """tests/host_softmax_harness.cpp with fmhip_host.cpp under AddressSanitizer and UBSan (a program of its own; no preloading)
    recomputes every recorded table — np.log(w / w.sum()).astype(float32) — bit for bit; a record with one number changed fails."""
    exe = str(tmp_path / "host_softmax_harness")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-pthread",
           os.path.join(ROOT, "tests", "host_softmax_harness.cpp"), os.path.join(ROOT, "sparkfm_amd", "csrc", "fmhip_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0 and b"sanitize" in r.stderr and b"cannot find" in r.stderr:
        pytest.skip("no sanitizer runtime for g++ in this image")
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    path = str(tmp_path / "vectors.txt")
    n, lines = vectors(path)
    assert n == 8
    r = subprocess.run([exe, path], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert r.returncode == 0 and ("checks ok %d" % n).encode() in r.stdout, r.stderr.decode()[-3000:]
    # the program does compare: the last table entry of the first record moved by an ulp
    v = lines[0].split()
    bad_lines = [" ".join(v[:-1] + ["%08x" % (int(v[-1], 16) + 1)])] + lines[1:]
    bad = str(tmp_path / "bad.txt")
    open(bad, "w").write("\n".join(bad_lines) + "\n")
    r = subprocess.run([exe, bad], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=300)
    assert r.returncode == 1 and b"check failed" in r.stderr and b"checks ok" not in r.stdout


# ---- the twin's learning -----------------------------------------------------------------------------------------------------------

SETTINGS = dict(k=8, batch_pairs=128, eta=1.0, regw=1e-3, regv=1e-3, epochs=30)
# held-out NDCG@10 of the twin on aref.hard_task(3) after 30 epochs, by n_neg and (proposal, logq); untrained: 0.0326
RECORDED = {1: dict(uniform=0.1097, popularity=0.0930, popularity_logq=0.1016),
            4: dict(uniform=0.0982, popularity=0.0873, popularity_logq=0.1075),
            8: dict(uniform=0.1180, popularity=0.1104, popularity_logq=0.1202)}


def twin_run(T, n_neg, mode, seed=3):
    P = aref.task_problem(T, seed, SETTINGS["k"], n_neg)
    s0 = ref.State(P["w0"], P["w"], P["v"], 0.1)
    w = pref.popularity(P)
    table = None if mode == "uniform" else pref.alias_table(w)
    lq = sref.logq(w) if mode == "popularity_logq" else None
    s, _ = sref.epochs(s0.copy(), P, SETTINGS["epochs"], SETTINGS["batch_pairs"], SETTINGS["eta"], 0.0, SETTINGS["regw"], SETTINGS["regv"],
                       ref.Rule("logistic", True, 1e-10), lq=lq, table=table)
    return aref.twin_ndcg(T, P, s0), aref.twin_ndcg(T, P, s)


@pytest.mark.parametrize("n_neg", [1, 4, 8])
def test_twin_ndcg_on_the_harder_task(n_neg):
    """The numbers the README quotes, from the fp64 twin alone, with the settings of its logistic rows (test_host_bpr_adaptive.py —
    the softmax at n_neg = 1 IS that rule): k = 8, batches of 128 pairs, AdaGrad (eps 1e-10, initial accumulator 0.1) with
    eta = 1.0, regw = regv = 1e-3, 30 epochs, v ~ N(0, 0.05), one candidate per pair.  They are recorded, not presumed: with uniform or popularity negatives and at most 8 of them the sampled softmax stays
    near the uniform-BPR row (0.1004 at n_neg = 3) and far below the best of 8 (0.3064) and WARP (0.5554), whose negatives are
    chosen by the model; the 1 / |B| scaling gives an interaction's n pairs the step of one.  n_neg = 8 clears the untrained model
    (0.0326) by more than a factor of 2 under every proposal."""
    T = aref.hard_task(3)
    for mode, want in RECORDED[n_neg].items():
        before, after = twin_run(T, n_neg, mode)
        assert before == pytest.approx(0.0326, abs=1e-4)
        assert after == pytest.approx(want, abs=1e-4), (n_neg, mode, after)
        if n_neg == 8:
            assert after > 2 * before
