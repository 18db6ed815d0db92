"""The MCMC learner's attribute groups on the GPU (include/fmhip_mcmc_groups.h, HipMCMC(groups=...)): G = 1 is the ungrouped handle
bit for bit; the sampled sweep follows mcmc_groups_ref.py on every walk; without sampling a per-group lambda is HipALS (equal
lambdas) or the twin's means (distinct ones); the level schedule, seeds and the state round-trip; a classification handle; the
planted task groups are for; the refusals; RelationalData.meta(); the C++ mirror.  Shapes and inputs are test_gpu_mcmc.py's."""
import ctypes as C

import numpy as np
import pytest

import mcmc_groups_ref as G
import mcmc_ref as R
import probit_ref as P
from test_gpu_mcmc import assert_same_bits, cpp_rows, dataset, model, params, problem, ref_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def groups_of(fmhip, kind, a, shape):
    """Dense kinds: feature i is of group i % 3.  One-hot: the field id, the extras a third group, a fourth group without a feature.
    Quirk Q1's slot (the last id) is given group 0 and must not count.  -> (Metadata over n1 entries, G)"""
    n1 = a["n1"]
    if kind == "onehot":
        g = np.concatenate([np.full(sz, f, np.int32) for f, sz in enumerate(shape)] + [np.full(n1 - sum(shape), len(shape), np.int32)])
        n = len(shape) + 2
    else:
        g, n = (np.arange(n1) % 3).astype(np.int32), 3
    g[n1 - 1] = 0
    return fmhip.Metadata(n1).update(g, numAttrGroups=n), n


def set_env(monkeypatch, env):
    for name, value in env.items():
        monkeypatch.setenv(name, value)


def same_state(p, q):
    return p["alpha"] == q["alpha"] and np.array_equal(np.ravel(p["lambda"]), np.ravel(q["lambda"])) and np.array_equal(np.ravel(p["mu"]), np.ravel(q["mu"]))


# ---- 1. G = 1 is the ungrouped handle ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,n_rows,shape,k,env", [("lds", 2000, 25, 3, {}), ("onehot", 9000, (300, 200), 4, {"FMHIP_ALS_LEVELS": "1"})], ids=["lds", "levels"])
def test_one_group_is_the_ungrouped_handle_bit_for_bit(fmhip, monkeypatch, kind, n_rows, shape, k, env):
    set_env(monkeypatch, env)
    a = problem(kind, n_rows, shape, k)
    ds = dataset(fmhip, a)
    out = []
    for groups in (None, np.zeros(a["n1"], np.int32)):
        fm = model(fmhip, a, k)
        mcmc = fmhip.HipMCMC.run(seed=31, groups=groups)
        for _ in range(2):
            mcmc.learn(fm, ds)
        out.append(params(fm) + (mcmc.state,))
        if groups is not None:
            assert mcmc.state["lambda"].shape == (k + 1, 1) and mcmc.group_counts.tolist() == [len(np.unique(a["col"][a["col"] < a["n1"] - 1]))]
        mcmc.close()
        fm.close()
    assert_same_bits(out[0], out[1])
    assert same_state(out[0][3], out[1][3]) and out[0][3]["lambda"].shape == (k + 1,)
    ds.unpersist()


# ---- 2. sampled sweeps against the twin ----------------------------------------------------------------------------------------

SAMPLED = [("lds", 2000, 25, 3, 0, {}), ("lds", 10001, 300, 2, 0, {}), ("long", 11000, 60, 2, 0, {"FMHIP_ALS_LONG": "1"}), ("onehot", 30000, (500, 400), 2, 2, {})]


def assert_follows_twin(fm, got, st):
    """test_gpu_mcmc.py's tolerances, for its reasons: the same fp64 arithmetic plus a noise term whose error is a few ulp."""
    print("max |dv| %.3e |dw| %.3e |dw0| %.3e  alpha %.6f / %.6f" % (np.abs(fm.v - st.v).max(), np.abs(fm.w - st.w).max(), abs(fm.w0 - st.w0), got["alpha"], st.alpha))
    np.testing.assert_allclose(fm.v, st.v, rtol=1e-8, atol=1e-11)
    np.testing.assert_allclose(fm.w, st.w, rtol=1e-8, atol=1e-11)
    assert fm.w0 == pytest.approx(st.w0, rel=1e-9, abs=1e-12)
    assert got["alpha"] == pytest.approx(st.alpha, rel=1e-9)
    np.testing.assert_allclose(got["lambda"], st.lam, rtol=1e-9)
    np.testing.assert_allclose(got["mu"], st.mu, rtol=1e-9)


@pytest.mark.parametrize("kind,n_rows,shape,k,extra,env", SAMPLED, ids=["lds", "workgroup-walk", "every-column-chip-wide", "levels"])
def test_sampling_follows_the_grouped_twin(fmhip, monkeypatch, kind, n_rows, shape, k, extra, env):
    set_env(monkeypatch, env)
    a = problem(kind, n_rows, shape, k, extra)
    n1 = a["n1"]
    meta, n_groups = groups_of(fmhip, kind, a, shape)
    ds = dataset(fmhip, a)
    fm = model(fmhip, a, k)
    mcmc = fmhip.HipMCMC.run(seed=20261019, groups=meta)
    st = G.State(a["w0"], a["w"], a["v"], meta.attrGroup, n_groups)
    p = ref_problem(a)
    for it in range(3):
        mcmc.learn(fm, ds)
        sse = G.epoch(st, p, seed=20261019)
        assert mcmc.last_stats["train_rmse"] == pytest.approx(np.sqrt(sse / n_rows), rel=1e-9)
    got = mcmc.state
    assert got["lambda"].shape == (k + 1, n_groups) and got["iterations"] == 3
    assert_follows_twin(fm, got, st)
    counts = G.group_counts(st, p)
    assert mcmc.group_counts.tolist() == counts.tolist()
    if kind == "onehot":
        assert counts[3] == 0 and counts[0] == len(np.unique(a["col"][a["col"] < shape[0]]))       # an empty group; Q1's slot is not in m_0
        assert (got["lambda"][:, 3] > 0).all() and np.ptp(got["lambda"][:, 3]) > 0                  # ... drawn from its prior
    assert np.array_equal(fm.v[:, n1 - 1], a["v"][:, n1 - 1]) and fm.w[n1 - 1] == a["w"][n1 - 1]    # quirk Q1
    assert np.ptp(got["lambda"][0]) > 0
    mcmc.close()
    fm.close()
    ds.unpersist()


# ---- 3. no sampling: a per-group lambda ----------------------------------------------------------------------------------------

CASES = [("lds", 2000, 25, 3, {}), ("lds", 10001, 300, 2, {}), ("long", 12000, 40, 2, {"FMHIP_ALS_LONG": "1050"}), ("onehot", 9000, (300, 200), 4, {"FMHIP_ALS_LEVELS": "1"})]


@pytest.mark.parametrize("kind,n_rows,shape,k,env", CASES, ids=["lds-walk", "workgroup-walk", "long-and-short", "levels"])
def test_without_sampling_equal_lambdas_are_the_als_epoch_bit_for_bit(fmhip, monkeypatch, kind, n_rows, shape, k, env):
    """alpha = 1, mu = 0, every group's lambda = (regw, regv ...): no sum enters, only the lookup differs — two epochs leave HipALS's bits."""
    set_env(monkeypatch, env)
    a = problem(kind, n_rows, shape, k)
    meta, n_groups = groups_of(fmhip, kind, a, shape)
    ds = dataset(fmhip, a)
    fm = model(fmhip, a, k)
    fm.reg0, fm.regw, fm.regv = 0.01, 0.1, 5.0
    for _ in range(2):
        fmhip.HipALS.run().learn(fm, ds)
    als = params(fm)
    fm.close()
    fm = model(fmhip, a, k)
    mcmc = fmhip.HipMCMC.run(sample=False, reg0=0.01, groups=meta)
    lam = np.repeat(np.array([[0.1]] + [[5.0]] * k), n_groups, axis=1)
    mcmc.state = (1.0, lam, np.zeros((k + 1, n_groups)))
    for _ in range(2):
        mcmc.learn(fm, ds)
    assert_same_bits(params(fm), als)
    st = mcmc.state
    assert st["alpha"] == 1.0 and np.array_equal(st["lambda"], lam) and not st["mu"].any() and st["iterations"] == 2
    mcmc.close()
    fm.close()
    ds.unpersist()


def test_without_sampling_distinct_lambdas_are_the_twins_means(fmhip):
    kind, n_rows, shape, k = "lds", 2000, 25, 3
    a = problem(kind, n_rows, shape, k)
    meta, n_groups = groups_of(fmhip, kind, a, shape)
    ds = dataset(fmhip, a)
    fm = model(fmhip, a, k)
    lam = 0.05 + np.arange((k + 1) * n_groups, dtype=np.float64).reshape(k + 1, n_groups) ** 2
    mu = 0.01 * np.arange((k + 1) * n_groups, dtype=np.float64).reshape(k + 1, n_groups) - 0.03
    mcmc = fmhip.HipMCMC.run(sample=False, reg0=0.01, groups=meta)
    mcmc.state = (1.7, lam, mu)
    st = G.State(a["w0"], a["w"], a["v"], meta.attrGroup, n_groups)
    st.alpha, st.lam, st.mu = 1.7, lam.copy(), mu.copy()
    p = ref_problem(a)
    for _ in range(2):
        mcmc.learn(fm, ds)
        G.epoch(st, p, sample=False, reg0=0.01)
    got = mcmc.state
    assert np.array_equal(got["lambda"], lam) and np.array_equal(got["mu"], mu)
    assert_follows_twin(fm, got, st)
    mcmc.close()
    fm.close()
    ds.unpersist()


# ---- 4. the schedule ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_rows,sizes,extra,k", [(9000, (300, 200), 0, 4), (30000, (500, 400), 2, 2)])
def test_the_draws_do_not_depend_on_the_schedule(fmhip, monkeypatch, n_rows, sizes, extra, k):
    """FMHIP_ALS_LEVELS 1 against 0, two epochs: equal bits up to 10,000 rows, 1e-11 (w0: 1e-12) above — the ungrouped test's rule."""
    a = problem("onehot", n_rows, sizes, k, extra)
    meta, _ = groups_of(fmhip, "onehot", a, sizes)
    ds = dataset(fmhip, a)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("FMHIP_ALS_LEVELS", mode)
        fm = model(fmhip, a, k)
        mcmc = fmhip.HipMCMC.run(seed=77, groups=meta)
        for _ in range(2):
            mcmc.learn(fm, ds)
        out[mode] = params(fm) + (mcmc.state,)
        mcmc.close()
        fm.close()
    if n_rows <= 10000:
        assert_same_bits(out["1"], out["0"])
        assert same_state(out["1"][3], out["0"][3])
    else:
        assert abs(out["1"][0] - out["0"][0]) <= 1e-12 and np.abs(out["1"][1] - out["0"][1]).max() <= 1e-11 and np.abs(out["1"][2] - out["0"][2]).max() <= 1e-11
    ds.unpersist()


# ---- 5. determinism and the state ------------------------------------------------------------------------------------------------

def test_seeds_and_the_group_state(fmhip):
    kind, n_rows, shape, k = "lds", 2000, 25, 3
    a = problem(kind, n_rows, shape, k)
    meta, n_groups = groups_of(fmhip, kind, a, shape)
    ds = dataset(fmhip, a)

    def run(seed, epochs=2):
        fm = model(fmhip, a, k)
        mcmc = fmhip.HipMCMC.run(seed=seed, groups=meta)
        for _ in range(epochs):
            mcmc.learn(fm, ds)
        out = params(fm) + (mcmc.state,)
        mcmc.close()
        fm.close()
        return out
    one, again, other = run(5), run(5), run(6)
    assert_same_bits(one, again)
    assert same_state(one[3], again[3])
    assert one[0] != other[0] and (one[2][:, :-1] != other[2][:, :-1]).all() and (one[3]["lambda"] != other[3]["lambda"]).all() and (one[3]["mu"] != other[3]["mu"]).all()
    assert len(np.unique(one[3]["lambda"])) == (k + 1) * n_groups          # every (g, a) has a draw of its own
    # the state round-trips
    fm = model(fmhip, a, k)
    mcmc = fmhip.HipMCMC.run(seed=5, sample=False, groups=meta)
    mcmc.learn(fm, ds)
    lam, mu = 1.0 + np.arange((k + 1) * n_groups, dtype=np.float64).reshape(k + 1, n_groups), -0.01 * np.arange((k + 1) * n_groups, dtype=np.float64).reshape(k + 1, n_groups)
    mcmc.state = (2.5, lam, mu)
    got = mcmc.state
    assert got["alpha"] == 2.5 and np.array_equal(got["lambda"], lam) and np.array_equal(got["mu"], mu) and got["iterations"] == 1
    from sparkfm_amd import _ffi
    with pytest.raises(_ffi.FmhipError, match="lambda\\[1\\]\\[2\\]"):
        bad = lam.copy()
        bad[1, 2] = 0.0
        mcmc.state = (1.0, bad, mu)
    with pytest.raises(ValueError, match="shape"):
        mcmc.state = (1.0, lam[:, 0], mu[:, 0])
    assert np.array_equal(mcmc.state["lambda"], lam)
    # the state of one (g, a) enters the steps of group a's features of parameter group g, and nothing before them: from the same
    # start, everything the sweep visits before factor k - 1's first feature of group 1 keeps its bits, and that feature moves
    start = params(fm)
    mcmc.learn(fm, ds)
    base = params(fm)
    fm.w0, fm.w, fm.v = start
    lam2 = lam.copy()
    lam2[k, 1] *= 3.0
    mcmc.state = (2.5, lam2, mu)
    mcmc.learn(fm, ds)
    moved = params(fm)
    feats = np.unique(a["col"][a["col"] < a["n1"] - 1])
    first = int(feats[meta.attrGroup[feats] == 1][0])
    assert moved[0] == base[0] and np.array_equal(moved[1], base[1]) and np.array_equal(moved[2][:k - 1], base[2][:k - 1])
    assert np.array_equal(moved[2][k - 1, :first], base[2][k - 1, :first]) and moved[2][k - 1, first] != base[2][k - 1, first]
    mcmc.close()
    fm.close()
    ds.unpersist()
    # rows of one feature each: the columns share no row and the factors' h is zero, so the state of (w, group 1) moves the linear
    # weights of group 1's features and nothing else
    n1 = 13
    col = (np.arange(600) % (n1 - 1)).astype(np.int32)
    b = dict(row_ptr=np.arange(601, dtype=np.int64), col=col, val=np.full(600, 1.0), y=np.sin(np.arange(600.0)), n1=n1, w0=0.2,
             w=0.01 * np.arange(n1), v=0.01 * np.arange(2 * n1, dtype=np.float64).reshape(2, n1))
    grp = (np.arange(n1) % 2).astype(np.int32)
    ds = dataset(fmhip, b)
    res = []
    for scale in (1.0, 4.0):
        fm = model(fmhip, b, 2)
        mcmc = fmhip.HipMCMC.run(sample=False, groups=grp)
        lam = np.ones((3, 2))
        lam[0, 1] = scale
        mcmc.state = (1.0, lam, np.zeros((3, 2)))
        mcmc.learn(fm, ds)
        res.append(params(fm))
        mcmc.close()
        fm.close()
    assert res[0][0] == res[1][0] and np.array_equal(res[0][2], res[1][2])
    assert np.array_equal(res[0][1][grp == 0], res[1][1][grp == 0]) and (res[0][1][:n1 - 1][grp[:n1 - 1] == 1] != res[1][1][:n1 - 1][grp[:n1 - 1] == 1]).all()
    ds.unpersist()


# ---- 6. a classification handle ---------------------------------------------------------------------------------------------------

def test_classification_with_groups_follows_the_twin(fmhip):
    """Two epochs on labels cut at the median: the grouped twin on probit_ref's latent targets (alpha stays 1), test 2's tolerances."""
    kind, n_rows, shape, k = "lds", 2000, 25, 3
    a = P.median_cut(problem(kind, n_rows, shape, k))
    meta, n_groups = groups_of(fmhip, kind, a, shape)
    ds = dataset(fmhip, a)
    fm = model(fmhip, a, k)
    mcmc = fmhip.HipMCMC.run(seed=11, task="classification", groups=meta)
    st = G.State(a["w0"], a["w"], a["v"], meta.attrGroup, n_groups)
    p = ref_problem(a)
    for _ in range(2):
        mcmc.learn(fm, ds)
        ystar, _, _, _, _, margin = P.latent_targets(st, p, seed=11)
        print("smallest accept / reject margin %.3e" % margin)
        G.epoch(st, p, seed=11, y=ystar, draw_alpha=False)
        np.testing.assert_allclose(mcmc.latent_targets(), ystar, rtol=1e-8, atol=1e-11)
    got = mcmc.state
    assert got["alpha"] == 1.0
    assert_follows_twin(fm, got, st)
    mcmc.close()
    fm.close()
    ds.unpersist()


# ---- 7. what groups are for ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("task_seed,seed", [(1, 7), (1, 8), (2, 7), (2, 8)])
def test_planted_task_with_fields_of_different_scales(fmhip, task_seed, seed):
    """mcmc_groups_ref.planted_task: two one-hot fields (30, 40) + the spare slot, user w ~ N(0, 2^2), item w ~ N(0, 0.1^2), v ~ N(0, 1),
    noise 0.3, 600 / 300 rows, k = 2; 40 epochs, 15 burn-in.  The item group's lambda_w, averaged over the kept epochs, is at least 10 x
    the user group's (a broken lookup gives 1 x), and the grouped averaged test RMSE is below the ungrouped run's on the same seeds.
    The twin on the CPU, these four: ratio 47.1 / 48.3 / 79.8 / 62.9; grouped RMSE 0.4346 / 0.4229 / 0.3929 / 0.3796 against
    ungrouped 0.4754 / 0.4790 / 0.4128 / 0.4012."""
    tr, te = G.planted_task(task_seed)
    n1, k = tr["n1"], 2
    init = dict(n1=n1, w0=0.0, w=np.zeros(n1), v=np.random.default_rng(5).normal(0, 0.01, (k, n1)))
    ds, test = dataset(fmhip, tr), dataset(fmhip, te)
    res = {}
    for name, groups in (("grouped", fmhip.Metadata.fromFields((30, 40), dimension=n1)), ("ungrouped", None)):
        fm = model(fmhip, init, k)
        mcmc = fmhip.HipMCMC.run(seed=seed, test=test, burn_in=15, groups=groups)
        lam_w = np.zeros(2 if groups is not None else 1)
        for it in range(40):
            mcmc.learn(fm, ds)
            if it >= 15:
                lam_w += np.atleast_1d(mcmc.state["lambda"][0])
        assert mcmc.draws == 25
        res[name] = (mcmc.computeRMSE(), lam_w / 25)
        mcmc.close()
        fm.close()
    (rmse_g, lam_g), (rmse_u, lam_u) = res["grouped"], res["ungrouped"]
    print("task %d seed %d: grouped RMSE %.4f ungrouped %.4f  lambda_w user %.3f item %.3f (ratio %.1f)  ungrouped lambda_w %.3f"
          % (task_seed, seed, rmse_g, rmse_u, lam_g[0], lam_g[1], lam_g[1] / lam_g[0], lam_u[0]))
    assert lam_g[1] >= 10.0 * lam_g[0]
    assert rmse_g < rmse_u
    ds.unpersist()
    test.unpersist()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_handle_unchanged(fmhip):
    from sparkfm_amd import _ffi
    L = _ffi.load()
    kind, n_rows, shape, k = "lds", 2000, 25, 3
    a = problem(kind, n_rows, shape, k)
    n = a["n1"] - 1
    ds = dataset(fmhip, a)
    fm = model(fmhip, a, k)
    start = params(fm)
    h = C.c_void_p()
    assert L.fmhip_mcmc_create(fm.handle, ds.handle, None, None, C.byref(h)) == 0
    table = (np.arange(n) % 3).astype(np.int32)

    def state(grouped):
        g = 3 if grouped else 1
        alpha, it, lam, mu = C.c_double(), C.c_int64(), np.empty((k + 1) * g), np.empty((k + 1) * g)
        assert (L.fmhip_mcmc_get_group_state if grouped else L.fmhip_mcmc_get_state)(h, C.byref(alpha), _ffi.ptr(lam), _ffi.ptr(mu), C.byref(it)) == 0
        return alpha.value, lam.tolist(), mu.tolist(), it.value

    def info():
        g = C.c_int32()
        assert L.fmhip_mcmc_group_info(h, C.byref(g), None) == 0
        counts = np.empty(g.value, np.int64)
        assert L.fmhip_mcmc_group_info(h, None, _ffi.ptr(counts)) == 0
        return g.value, counts.tolist()

    for grouped in (False, True):
        if grouped:
            assert L.fmhip_mcmc_set_groups(h, _ffi.ptr(table), n, 3) == 0
            lam = np.arange(1.0, 1.0 + (k + 1) * 3)
            assert L.fmhip_mcmc_set_group_state(h, 2.0, _ffi.ptr(lam), _ffi.ptr(-lam)) == 0
        before, before_info = state(grouped), info()
        bad = table.copy()
        bad[17] = 3
        neg = table.copy()
        neg[4] = -1
        for args, code, words in (((None, n, 3), -1, b"group table is NULL"), ((_ffi.ptr(table), n - 1, 3), -1, b"num_attribute = %d" % n),
                                  ((_ffi.ptr(table), n + 1, 3), -1, b"n = %d" % (n + 1)), ((_ffi.ptr(table), n, 0), -1, b"n_groups = 0"),
                                  ((_ffi.ptr(bad), n, 3), -1, b"feature 17 has group id 3"), ((_ffi.ptr(neg), n, 3), -1, b"feature 4 has group id -1"),
                                  ((_ffi.ptr(table), n, 4097), -5, b"FMHIP_MCMC_MAX_GROUPS")):
            assert L.fmhip_mcmc_set_groups(h, *args) == code and words in L.fmhip_last_error(), (args, L.fmhip_last_error())
            assert state(grouped) == before and info() == before_info
            assert_same_bits(params(fm), start)
    # the old state calls refuse a handle with G > 1 and name the group calls; alpha and the iterations alone are still read
    lam = np.ones(k + 1)
    assert L.fmhip_mcmc_get_state(h, None, _ffi.ptr(lam), None, None) == -1 and b"fmhip_mcmc_get_group_state" in L.fmhip_last_error()
    assert L.fmhip_mcmc_set_state(h, 1.0, _ffi.ptr(lam), _ffi.ptr(lam)) == -1 and b"fmhip_mcmc_set_group_state" in L.fmhip_last_error()
    alpha = C.c_double()
    assert L.fmhip_mcmc_get_state(h, C.byref(alpha), None, None, None) == 0 and alpha.value == 2.0
    assert state(True) == before
    # set_groups resets the state; after the first epoch it is refused
    assert L.fmhip_mcmc_set_groups(h, _ffi.ptr(table), n, 3) == 0
    assert state(True) == (2.0, [1.0] * ((k + 1) * 3), [0.0] * ((k + 1) * 3), 0)
    assert info() == (3, np.bincount(table[np.unique(a["col"][a["col"] < n])], minlength=3).tolist())
    assert L.fmhip_mcmc_epoch(h, None) == 0
    after = state(True)
    assert L.fmhip_mcmc_set_groups(h, _ffi.ptr(table), n, 3) == -1 and b"before the handle's first epoch" in L.fmhip_last_error()
    assert L.fmhip_mcmc_set_groups(h, _ffi.ptr(table), n, 1) == -1 and state(True) == after and after[3] == 1
    assert L.fmhip_mcmc_destroy(h) == 0
    # through HipMCMC: a table shorter than the model raises when the handle is made, the model untouched
    fm2 = model(fmhip, a, k)
    with pytest.raises(ValueError, match="groups holds 5 ids"):
        fmhip.HipMCMC.run(groups=np.zeros(5, np.int32)).learn(fm2, ds)
    assert_same_bits(params(fm2), start)
    fm2.close()
    fm.close()
    ds.unpersist()


# ---- 9. a block is a group ----------------------------------------------------------------------------------------------------------

def test_relational_meta_feeds_the_learner(fmhip):
    rng = np.random.default_rng(3)
    n, users, items = 400, 30, 20
    ublock = [([u, users + items + u % 5], [1.0, 0.5]) for u in range(users)]                 # ids 0..29 and 50..54
    iblock = [([users + i], [1.0]) for i in range(items)]                                     # ids 30..49
    pcol = (60 + rng.integers(0, 4, n)).astype(np.int32)                                      # ids 60..63 (63: the spare slot)
    pcol[:4] = [60, 61, 62, 63]
    plain = fmhip.DataSet(np.arange(n + 1, dtype=np.int64), pcol, np.ones(n), np.zeros(n))
    rd = fmhip.RelationalData(rng.normal(0, 1, n), [fmhip.Relation(ublock, rng.integers(0, users, n)), fmhip.Relation(iblock, rng.integers(0, items, n))],
                              plain=plain)
    meta = rd.meta()
    flat = rd.expand().cache()
    assert meta.numAttrGroups == 3 and meta.dimension == flat.dimension == 63
    fm = fmhip.FMModel(flat.dimension, 2, seed=1)
    mcmc = fmhip.HipMCMC.run(seed=2, groups=meta)
    mcmc.learn(fm, flat)
    used = np.unique(flat.col)
    want = [int(np.sum((used < 30) | ((used >= 50) & (used < 55)))), int(np.sum((used >= 30) & (used < 50))), int(np.sum((used >= 60) & (used < 63)))]
    assert mcmc.group_counts.tolist() == want and want[2] == 3 and mcmc.state["lambda"].shape == (3, 3)
    mcmc.close()
    fm.close()
    flat.unpersist()


# ---- 10. the C++ mirror ---------------------------------------------------------------------------------------------------------------

def test_cpp_mcmc_groups_matches_python(fmhip, tmp_path):
    """tests/cpp_mcmc_groups.cpp (include/sparkfm.hpp's HipMCMC with setGroups) against the Python mirror: hex floats equal."""
    import os
    import subprocess
    from sparkfm_amd import _build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_mcmc_groups")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_mcmc_groups.cpp"), "-L" + _build.LIBDIR, "-lfmhip",
                           "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.decode().splitlines()}
    hexes = lambda name: [float.fromhex(t) for t in got[name]]      # noqa: E731
    n1, k = 40, 3
    a = dict(n1=n1, w0=0.1, w=np.array([0.02 * ((i % 7) - 3) for i in range(n1)]),
             v=np.array([[0.01 * ((f * 7 + i * 3) % 11 - 5) for i in range(n1)] for f in range(k)]))
    ds = dataset(fmhip, cpp_rows(400, 0))
    fm = model(fmhip, a, k)
    mcmc = fmhip.HipMCMC.run(seed=12, groups=(np.arange(n1) % 3).astype(np.int32))
    for _ in range(3):
        mcmc.learn(fm, ds)
    st = mcmc.state
    assert hexes("w0") == [fm.w0] and hexes("w") == fm.w.tolist() and hexes("v") == fm.v.reshape(-1, order="F").tolist()
    assert hexes("alpha") == [st["alpha"]] and hexes("lambda") == st["lambda"].reshape(-1).tolist() and hexes("mu") == st["mu"].reshape(-1).tolist()
    assert [int(c) for c in got["counts"]] == mcmc.group_counts.tolist() and got["groups"] == ["3", "3"]
    assert np.ptp(st["lambda"][0]) > 0
    mcmc.close()
    fm.close()
    ds.unpersist()
