"""The MCMC learner over relational data (include/fmhip_mcmc_relational.h) on the device: HipBlockMCMC on a RelationalData against the fp64
twin by block caches (mcmc_blocks_ref.py) and against the flat sampler on expand(); the two walks; T and quirk Q1; relational and flat
test sets; determinism and the (k + 1, P) state; the refusals; include/sparkfm.hpp.

Tolerances: against the twin, test_gpu_mcmc.py's for the same arithmetic (mcmc_blocks_cases.TWIN_*); against the flat sampler, 100 x the
distance between the two twins measured on the CPU (mcmc_blocks_cases.RECORDED), floored at the twin's."""
import numpy as np
import pytest

import mcmc_blocks_cases as K
import mcmc_blocks_ref as B
import probit_ref as PR

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def relation(fmhip, part, name):
    return fmhip.Relation((part.row_ptr, part.col.astype(np.int32), part.val), part.mapping.astype(np.int32), name=name)


def relational(fmhip, rp, share=None, **kw):
    """The twin's Relational as a RelationalData; share: the RelationalData whose blocks this one uses under its own mappings."""
    rels, plain = [], None
    for i, part in enumerate(rp.parts):
        if part.mapping is None:
            plain = fmhip.DataSet(part.row_ptr, part.col.astype(np.int32), part.val, rp.y, batch_rows=kw.get("batch_rows", 0))
        elif share is not None:
            rels.append(share.relations[i].remap(part.mapping.astype(np.int32)))
        else:
            rels.append(relation(fmhip, part, "part%d" % i))
    return fmhip.RelationalData(rp.y, rels, plain=plain, **kw)


def model(fmhip, prob):
    fm = fmhip.FMModel(prob["n1"] - 1, prob["k"])
    fm.w0, fm.w, fm.v = prob["w0"], prob["w"], prob["v"]
    return fm


def params(fm):
    return fm.w0, fm.w.copy(), np.array(fm.v)


def assert_same_bits(p, q):
    assert p[0] == q[0]
    np.testing.assert_array_equal(p[1], q[1])
    np.testing.assert_array_equal(p[2], q[2])


def learner(fmhip, by_parts, task, sample, **kw):
    mcmc = fmhip.HipBlockMCMC.run(seed=K.SEED, sample=sample, task=task, groups="parts" if by_parts else None, reg0=0.0 if sample else K.REG0, **kw)
    if not sample:
        lam = np.full(4, K.REGV)
        lam[0] = K.REGW
        mcmc.state = (1.0, lam, np.zeros(4))
    return mcmc


def close(a, b, rtol, atol, what):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=what)


def assert_follows(fm, state, st, what):
    """w, v to rtol 1e-8 / atol 1e-11; w0, alpha, lambda, mu to 1e-9 relative — against a twin's State."""
    close(fm.w, st.w, K.TWIN_RTOL, K.TWIN_ATOL, what + " w")
    close(np.array(fm.v), st.v, K.TWIN_RTOL, K.TWIN_ATOL, what + " v")
    assert abs(fm.w0 - st.w0) <= K.TWIN_REL * abs(st.w0), (what, fm.w0, st.w0)
    assert abs(state["alpha"] - st.alpha) <= K.TWIN_REL * st.alpha, (what, state["alpha"], st.alpha)
    close(np.reshape(state["lambda"], st.lam.shape), st.lam, K.TWIN_REL, 0.0, what + " lambda")
    close(np.reshape(state["mu"], st.mu.shape), st.mu, K.TWIN_REL, 0.0, what + " mu")


def assert_follows_params(p, st):
    close(p[1], st.w, K.TWIN_RTOL, K.TWIN_ATOL, "w")
    close(p[2], st.v, K.TWIN_RTOL, K.TWIN_ATOL, "v")
    assert abs(p[0] - st.w0) <= K.TWIN_REL * abs(st.w0)


@pytest.fixture(scope="module")
def problems():
    """The base shape once per task (and the 700-row one whose hot item's list is summed in chunks): shared, never changed."""
    return {"regression": B.base_problem(K.SEED), "classification": B.base_problem(K.SEED, classification=True),
            "chunked": B.base_problem(K.SEED, n_rows=700)}


# ---- 1. the twin --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("by_parts,task,sample", K.CASES, ids=K.IDS)
def test_follows_the_block_twin(fmhip, problems, by_parts, task, sample):
    """3 epochs on the base shape against mcmc_blocks_ref; classification: latent_targets() to 1e-8 as well."""
    prob = problems[task]
    rd, fm = relational(fmhip, prob["train"]).cache(), model(fmhip, prob)
    mcmc = learner(fmhip, by_parts, task, sample)
    for _ in range(K.EPOCHS):
        mcmc.learn(fm, rd)
    st = K.run_blocks(prob, by_parts, task, sample)
    assert_follows(fm, mcmc.state, st, "block twin")
    assert np.abs(fm.w - prob["w"]).max() > 0.1
    if task == "classification":
        close(mcmc.latent_targets(), st.ystar, 1e-8, 1e-8, "latent targets")
    else:
        np.testing.assert_array_equal(mcmc.latent_targets(), prob["train"].y)
    mcmc.close()
    rd.unpersist()


def test_a_long_list_is_summed_in_chunks(fmhip, problems):
    """700 rows: the hot item is referenced by more than FMHIP_RELATIONAL_SUM_CUT = 256 rows, its caches are chunk sums added in order."""
    prob = problems["chunked"]
    assert np.bincount(prob["train"].parts[1].mapping).max() > 256
    rd, fm = relational(fmhip, prob["train"]).cache(), model(fmhip, prob)
    mcmc = learner(fmhip, False, "regression", True)
    for _ in range(K.EPOCHS):
        mcmc.learn(fm, rd)
    assert_follows(fm, mcmc.state, K.run_blocks(prob, False, "regression", True), "chunked")
    mcmc.close()
    rd.unpersist()


# ---- 2. the flat sampler on expand() -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("by_parts,task,sample", K.CASES, ids=K.IDS)
def test_follows_the_flat_sampler_on_the_expanded_rows(fmhip, problems, by_parts, task, sample):
    """The same runs against HipMCMC on expand() with the same seed (groups = relational.meta() by parts), and without sampling against
    HipALS on expand(): both routes round the same algebra differently."""
    case = (by_parts, task, sample)
    prob = problems[task]
    rd, fm = relational(fmhip, prob["train"]).cache(), model(fmhip, prob)
    mcmc = learner(fmhip, by_parts, task, sample)
    for _ in range(K.EPOCHS):
        mcmc.learn(fm, rd)
    flat, fm2 = rd.expand().cache(), model(fmhip, prob)
    if sample:
        other = fmhip.HipMCMC.run(seed=K.SEED, task=task, groups=rd.meta() if by_parts else None)
    else:
        other = fmhip.HipALS.run()
        fm2.reg0, fm2.regw, fm2.regv = K.REG0, K.REGW, K.REGV
    for _ in range(K.EPOCHS):
        other.learn(fm2, flat)
    for name, got, want in (("w", fm.w, fm2.w), ("v", np.array(fm.v), np.array(fm2.v))):
        rtol, atol = K.flat_tolerance(case, name)
        close(got, want, rtol, atol, "flat " + name)
    assert abs(fm.w0 - fm2.w0) <= K.flat_tolerance(case, "w0") * abs(fm2.w0)
    if sample:
        a, b = mcmc.state, other.state
        assert abs(a["alpha"] - b["alpha"]) <= K.flat_tolerance(case, "alpha") * b["alpha"]
        for name in ("lambda", "mu"):
            close(np.ravel(a[name]), np.ravel(b[name]), K.flat_tolerance(case, name), 0.0, "flat " + name)
        assert mcmc.group_counts.tolist() == other.group_counts.tolist()
        other.close()
    mcmc.close()
    flat.unpersist()
    rd.unpersist()


# ---- 3. the two walks ---------------------------------------------------------------------------------------------------------------

def test_the_level_walk_and_the_workgroup_walk_agree(fmhip, problems, monkeypatch):
    """FMHIP_ALS_LEVELS=0 (one workgroup over the block's columns in order) against =1 (a wave per column of a level): parameters
    within 1e-11, w0 within 1e-12 — the flat schedule test's bounds; the walks differ in the order of a column's sum only."""
    prob = problems["regression"]
    got = []
    for levels in ("0", "1"):
        monkeypatch.setenv("FMHIP_ALS_LEVELS", levels)
        rd, fm = relational(fmhip, prob["train"]).cache(), model(fmhip, prob)
        mcmc = learner(fmhip, True, "regression", True)
        for _ in range(K.EPOCHS):
            mcmc.learn(fm, rd)
        got.append(params(fm))
        mcmc.close()
        rd.unpersist()
    assert abs(got[0][0] - got[1][0]) <= 1e-12
    assert np.abs(got[0][1] - got[1][1]).max() <= 1e-11 and np.abs(got[0][2] - got[1][2]).max() <= 1e-11
    assert np.abs(got[0][2] - prob["v"]).max() > 1e-3


def test_a_long_block_column_takes_the_workgroup_walk_behind_its_level(fmhip, problems, monkeypatch):
    """The level walk with FMHIP_ALS_LONG = 4: every history and genre column of four entries or more is left out of its level's
    launch and stepped by the 1024-thread workgroup walk behind it (the plain part's columns take the flat walk's chip-wide step).
    Against the level walk at the default threshold: the schedule test's bounds — only the order of a column's sum differs."""
    prob = problems["regression"]
    users, items, _ = prob["train"].parts
    assert max(np.diff(users.cptr).max(), np.diff(items.cptr).max()) >= 4 and np.diff(users.cptr).min() < 4
    got = []
    monkeypatch.setenv("FMHIP_ALS_LEVELS", "1")
    for long_col in (None, "4"):
        if long_col:
            monkeypatch.setenv("FMHIP_ALS_LONG", long_col)
        rd, fm = relational(fmhip, prob["train"]).cache(), model(fmhip, prob)
        mcmc = learner(fmhip, True, "regression", True)
        for _ in range(K.EPOCHS):
            mcmc.learn(fm, rd)
        got.append(params(fm))
        mcmc.close()
        rd.unpersist()
    assert abs(got[0][0] - got[1][0]) <= 1e-12
    assert np.abs(got[0][1] - got[1][1]).max() <= 1e-11 and np.abs(got[0][2] - got[1][2]).max() <= 1e-11
    assert_follows_params(got[1], K.run_blocks(prob, True, "regression", True))


# ---- 4. T and quirk Q1 --------------------------------------------------------------------------------------------------------------

def test_untrained_features_keep_their_bits(fmhip, problems):
    """The feature stored only in the two user rows nobody references — and those two users' own ids — are not in T: their parameters
    keep their bits and they do not count; neither does the last slot (id = num_attribute, stored in one plain row)."""
    prob = problems["regression"]
    rp, lonely, last = prob["train"], prob["lonely"], prob["n1"] - 1
    assert lonely in rp.parts[0].feat and last in rp.parts[2].feat
    rd, fm = relational(fmhip, rp).cache(), model(fmhip, prob)
    want = B.group_counts(rp, prob["n1"] - 1)
    assert want.tolist() == [len(rp.parts[0].feat) - 3, len(rp.parts[1].feat), len(rp.parts[2].feat) - 1]
    untouched = [B.USERS - 2, B.USERS - 1, lonely, last]
    for by_parts in (False, True):
        mcmc = learner(fmhip, by_parts, "regression", True)
        for _ in range(2):
            mcmc.learn(fm, rd)
        assert mcmc.group_counts.tolist() == (want.tolist() if by_parts else [int(want.sum())])
        mcmc.close()
    for i in untouched:
        assert fm.w[i] == prob["w"][i]
        np.testing.assert_array_equal(np.array(fm.v)[:, i], prob["v"][:, i])
    assert np.abs(np.delete(fm.w, untouched) - np.delete(prob["w"], untouched)).min() > 0
    rd.unpersist()


# ---- 5. test sets -------------------------------------------------------------------------------------------------------------------

def auc(p, y):
    order = np.argsort(p, kind="stable")
    ranks = np.empty(len(p))
    ranks[order] = np.arange(1, len(p) + 1)
    for v in np.unique(p):                      # ties share their mean rank
        ranks[p == v] = ranks[p == v].mean()
    pos = y > 0
    return (ranks[pos].sum() - pos.sum() * (pos.sum() + 1) / 2.0) / (pos.sum() * (~pos).sum())


@pytest.mark.parametrize("task", ["regression", "classification"])
@pytest.mark.parametrize("kind", ["relational", "flat"])
def test_test_sets(fmhip, problems, task, kind):
    """4 epochs, burn_in = 1, a relational test set over the train set's blocks (remap) or its flat expansion: predictions() is the mean
    of the twin's 3 kept draws to 1e-8, the scores agree with the twin's, fm.predict(test) is last_predictions() to 1e-4 (fp32)."""
    prob = problems[task]
    rd = relational(fmhip, prob["train"]).cache()
    rt = relational(fmhip, prob["test"], share=rd)
    test = rt.cache() if kind == "relational" else rt.expand().cache()
    fm = model(fmhip, prob)
    mcmc = learner(fmhip, True, task, True, test=test, burn_in=1)
    for _ in range(4):
        mcmc.learn(fm, rd)
    kept = []
    K.run_blocks(prob, True, task, True, epochs=4, keep=kept)
    mean, y = np.mean(kept[1:], axis=0), prob["test"].y
    assert mcmc.draws == 3
    close(mcmc.predictions(), mean, 1e-8, 1e-8, "averaged predictions")
    close(mcmc.last_predictions(), kept[-1], 1e-8, 1e-8, "last predictions")
    score = np.asarray(fm.predict(test), np.float64)
    close(PR.normal_cdf(score) if task == "classification" else score, mcmc.last_predictions(), 0.0, 1e-4, "fm.predict")
    if task == "classification":
        assert abs(mcmc.computeLogLoss() - PR.logloss(mean, y)) <= 1e-8
        assert mcmc.computeAccuracy() == PR.accuracy(mean, y)
        assert abs(mcmc.computeAUC() - auc(mean, y)) <= 1e-6
    else:
        assert abs(mcmc.computeRMSE() - float(np.sqrt(np.mean((mean - y) ** 2)))) <= 1e-8
    mcmc.close()
    test.unpersist()
    rd.unpersist()


def test_clip_labels_reads_the_relational_labels(fmhip, problems):
    """clip="labels" clamps every draw's test prediction to the range of relational.y: with the train labels cut to their 30 % - 70 %
    quantiles the clamp binds (21 of the twin's 360 kept test predictions lie outside), and predictions() is the mean of the twin's
    CLAMPED draws to 1e-8."""
    prob = problems["regression"]
    rp = prob["train"]
    lo, hi = np.quantile(rp.y, [0.3, 0.7])
    cut = dict(prob, train=B.Relational(np.clip(rp.y, lo, hi), rp.parts))
    rd = relational(fmhip, cut["train"]).cache()
    assert rd.y.min() == lo and rd.y.max() == hi
    test = relational(fmhip, prob["test"], share=rd).cache()
    fm = model(fmhip, prob)
    mcmc = learner(fmhip, False, "regression", True, test=test, burn_in=1, clip="labels")
    for _ in range(4):
        mcmc.learn(fm, rd)
    kept = []
    K.run_blocks(cut, False, "regression", True, epochs=4, keep=kept)
    kept = np.array(kept[1:])
    assert ((kept < lo) | (kept > hi)).sum() > 10
    close(mcmc.predictions(), np.clip(kept, lo, hi).mean(axis=0), 1e-8, 1e-8, "clamped mean")
    assert mcmc.predictions().min() >= lo and mcmc.predictions().max() <= hi
    assert np.abs(mcmc.predictions() - kept.mean(axis=0)).max() > 1e-3
    mcmc.close()
    test.unpersist()
    rd.unpersist()


# ---- 6. determinism and the state --------------------------------------------------------------------------------------------------

def test_runs_repeat_bit_for_bit_and_the_state_round_trips(fmhip, problems):
    prob = problems["regression"]
    rd = relational(fmhip, prob["train"]).cache()
    got = []
    for _ in range(2):
        fm, mcmc = model(fmhip, prob), learner(fmhip, True, "regression", True)
        for _ in range(2):
            mcmc.learn(fm, rd)
        got.append((params(fm), mcmc.state))
        mcmc.close()
    assert_same_bits(got[0][0], got[1][0])
    a, b = got[0][1], got[1][1]
    assert a["alpha"] == b["alpha"] and np.array_equal(a["lambda"], b["lambda"]) and np.array_equal(a["mu"], b["mu"])
    assert a["lambda"].shape == (4, 3) == a["mu"].shape and a["iterations"] == 2 and np.ptp(a["lambda"][0]) > 0
    # the state as set is the state read back, and a run from it repeats
    runs = []
    for _ in range(2):
        fm, mcmc = model(fmhip, prob), learner(fmhip, True, "regression", True)
        mcmc.state = (a["alpha"], a["lambda"], a["mu"])
        mcmc.learn(fm, rd)
        runs.append(params(fm))
        back = mcmc.state
        assert back["lambda"].shape == (4, 3)
        with pytest.raises(ValueError, match="shape"):
            mcmc.state = (1.0, np.ones(4), np.zeros(4))
        mcmc.close()
    assert_same_bits(runs[0], runs[1])
    fm, mcmc = model(fmhip, prob), learner(fmhip, True, "regression", False)
    mcmc.state = (a["alpha"], a["lambda"], a["mu"])
    mcmc._handle(fm, rd)
    back = mcmc.state
    assert back["alpha"] == a["alpha"] and np.array_equal(back["lambda"], a["lambda"]) and np.array_equal(back["mu"], a["mu"])
    mcmc.close()
    rd.unpersist()


def test_with_relation_fits_by_blocks(fmhip, problems):
    """FM(plain rows, k).withRelation([users, items]).learnWith(HipBlockMCMC...) is the fit loop over the RelationalData it builds: the bits
    of three learn() calls on that RelationalData from the same start."""
    prob = problems["regression"]
    rp = prob["train"]
    rd, fm = relational(fmhip, rp).cache(), model(fmhip, prob)
    mcmc = learner(fmhip, True, "regression", True)
    for _ in range(K.EPOCHS):
        mcmc.learn(fm, rd)
    want, state = params(fm), mcmc.state
    mcmc.close()
    plain = rp.parts[2]
    rows = fmhip.DataSet(plain.row_ptr, plain.col.astype(np.int32), plain.val, rp.y, batch_rows=0)
    mcmc = learner(fmhip, True, "regression", True)
    fit = fmhip.FM(rows, prob["k"], maxIteration=K.EPOCHS).withRelation(rd.relations)
    got = fit.learnWith(mcmc, init=(prob["w0"], prob["w"], prob["v"]))
    assert_same_bits(params(got), want)
    assert np.array_equal(mcmc.state["lambda"], state["lambda"]) and len(fit.rmse_history) == K.EPOCHS
    mcmc.close()
    rd.unpersist()


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_model_unchanged(fmhip, problems):
    from sparkfm_amd import _ffi
    L = _ffi.load()
    prob = problems["regression"]
    rp = prob["train"]
    fm = model(fmhip, prob)
    start = params(fm)

    def refused(train, code, words, exc=None, **kw):
        mcmc = fmhip.HipBlockMCMC.run(**kw)
        with pytest.raises(exc or _ffi.FmhipError, match=words) as err:
            mcmc.learn(fm, train)
        if exc is None:
            assert err.value.code == code
        assert_same_bits(params(fm), start)
        mcmc.close()
    ok = relational(fmhip, rp).cache()
    # the parts' id ranges interleave: the item block's genres moved in front of the users' history
    users, items, plain = rp.parts
    moved = np.where(items.col >= 78, items.col - 78 + 41, items.col)
    shifted = np.where((users.col >= 41) & (users.col < 52), users.col + 100, users.col)
    inter = B.Relational(rp.y, [B.Block(users.row_ptr, shifted, users.val, users.mapping), B.Block(items.row_ptr, moved, items.val, items.mapping), plain])
    wide = fmhip.FMModel(200, prob["k"])
    wide.w0, wide.w, wide.v = 0.3, np.linspace(-1.0, 1.0, 201), np.linspace(-0.5, 0.5, 201 * prob["k"]).reshape(prob["k"], 201)
    wide_start = params(wide)
    mcmc = fmhip.HipBlockMCMC.run()
    with pytest.raises(_ffi.FmhipError, match="feature 41 of relation 1 lies inside the id range of relation 0") as err:
        mcmc.learn(wide, relational(fmhip, inter).cache())
    assert err.value.code == -5
    assert_same_bits(params(wide), wide_start)
    mcmc.close()
    wide.close()
    # a part with a dense hot block (asked for by name), a part with row-blocked transposes
    hot_plain = fmhip.DataSet(plain.row_ptr, plain.col.astype(np.int32), plain.val, rp.y, batch_rows=0, hot_block=4).cache()
    assert len(hot_plain.layout()["hot_ids"]) > 0
    hot = fmhip.RelationalData(rp.y, [relation(fmhip, users, "u"), relation(fmhip, items, "i")], plain=hot_plain)
    refused(hot.cache(), -5, "the train set, the plain part: .*hot block")
    blocked = fmhip.DataSet(items.row_ptr, items.col.astype(np.int32), items.val, np.zeros(items.n_rows), batch_rows=0, row_block_rows=8).cache()
    rowb = fmhip.RelationalData(rp.y, [relation(fmhip, users, "u"), fmhip.Relation(blocked, items.mapping.astype(np.int32))],
                                plain=fmhip.DataSet(plain.row_ptr, plain.col.astype(np.int32), plain.val, rp.y, batch_rows=0))
    refused(rowb.cache(), -5, "the train set, relation 1: .*row blocks")
    # more than one batch
    refused(relational(fmhip, rp, batch_rows=100).cache(), -5, "the train set has 3 batches")
    # a block row that stores a feature twice
    dup = fmhip.RelationalData(rp.y, [fmhip.Relation([([0, 40, 40], [1.0, 0.5, 0.5]), ([1], [1.0])], (users.mapping % 2).astype(np.int32)),
                                      relation(fmhip, items, "items")])
    refused(dup.cache(), -5, "the train set, relation 0: .*twice")
    # weights: the relational dataset itself refuses a weighted part
    with pytest.raises(_ffi.FmhipError, match="weight"):
        fmhip.RelationalData(rp.y, [relation(fmhip, users, "u"), relation(fmhip, items, "i")],
                             plain=fmhip.DataSet(plain.row_ptr, plain.col.astype(np.int32), plain.val, rp.y, batch_rows=0, weights=np.ones(rp.n_rows))).cache()
    # a model set to the logistic loss, or to pairs
    assert L.fmhip_model_set_loss(fm.handle, _ffi.LOSS_LOGISTIC) == 0
    refused(ok, -5, "the train set, relation 0: .*logistic loss")
    assert L.fmhip_model_set_loss(fm.handle, _ffi.LOSS_SQUARED) == 0 and L.fmhip_model_set_pairing(fm.handle, _ffi.PAIRING_ADJACENT) == 0
    refused(ok, -5, "pairs of rows")
    assert L.fmhip_model_set_pairing(fm.handle, _ffi.PAIRING_NONE) == 0
    # a general group table; 'parts' with flat rows; both kinds of test set through the C call; set_groups on a relational handle
    refused(ok, 0, "groups='parts'", exc=ValueError, groups=np.zeros(prob["n1"], np.int32))
    refused(ok, 0, "groups='parts'", exc=ValueError, groups=ok.meta())
    flat = ok.expand().cache()
    refused(flat, 0, "sweeps the blocks of a RelationalData", exc=TypeError, groups="parts")
    refused(flat, 0, "sweeps the blocks of a RelationalData", exc=TypeError, test=ok)
    # ... and HipMCMC itself still takes flat rows only, as a train and as a test set
    with pytest.raises(TypeError, match="RelationalData.*expand"):
        fmhip.HipMCMC.run().learn(fm, ok)
    with pytest.raises(TypeError, match="RelationalData.*expand"):
        fmhip.HipMCMC.run(test=ok)
    assert_same_bits(params(fm), start)
    import ctypes as C
    h = C.c_void_p()
    assert L.fmhip_mcmc_create_relational(fm.handle, ok.rel_handle, ok.rel_handle, flat.handle, None, None, 0, C.byref(h)) == -1
    assert h.value is None and b"at most one" in L.fmhip_last_error()
    mcmc = fmhip.HipBlockMCMC.run()
    mcmc.learn(fm, ok)                          # ... and afterwards it trains
    assert np.abs(fm.v - start[2]).max() > 1e-3
    table = np.zeros(prob["n1"] - 1, np.int32)
    assert L.fmhip_mcmc_set_groups(mcmc._h, _ffi.ptr(table), len(table), 2) == -5 and b"its parts" in L.fmhip_last_error()
    mcmc.close()
    fm.close()


# ---- 8. the C++ mirror --------------------------------------------------------------------------------------------------------------

def cpp_problem():
    """The integer formulas of tests/cpp_mcmc_relational.cpp: 6 users (id + one of 3 history features), 5 items (id + one of 2 genres),
    2 plain features; 60 train and 20 test rows."""
    def rows(n, shift):
        umap = np.array([(3 * (j + shift) + 1) % 6 for j in range(n)], np.int32)
        imap = np.array([(7 * (j + shift) + 2) % 5 for j in range(n)], np.int32)
        pcol = np.array([[16, 17] for _ in range(n)], np.int32).reshape(-1)
        pval = np.array([[0.25 * (((j + shift) % 5) - 2), 0.5 * (((j + shift) % 3) - 1) + 0.125] for j in range(n)]).reshape(-1)
        y = np.array([0.5 * (((j + shift) * 5) % 9) - 1.0 for j in range(n)])
        return umap, imap, (np.arange(0, 2 * n + 1, 2, dtype=np.int64), pcol, pval), y
    ublock = (np.arange(0, 13, 2, dtype=np.int64), np.array([[u, 6 + u % 3] for u in range(6)], np.int32).reshape(-1),
              np.array([[1.0, 0.5 + 0.25 * (u % 2)] for u in range(6)]).reshape(-1))
    iblock = (np.arange(0, 11, 2, dtype=np.int64), np.array([[9 + i, 14 + i % 2] for i in range(5)], np.int32).reshape(-1),
              np.array([[1.0, 0.75] for i in range(5)]).reshape(-1))
    return ublock, iblock, rows(60, 0), rows(20, 3)


def test_cpp_mcmc_relational_matches_python(fmhip, tmp_path):
    """tests/cpp_mcmc_relational.cpp (include/sparkfm.hpp's HipMCMC over a RelationalData) against the Python mirror: hex floats equal."""
    import os
    import subprocess
    from sparkfm_amd import _build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cpp_mcmc_relational")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp_mcmc_relational.cpp"), "-L" + _build.LIBDIR, "-lfmhip",
                           "-Wl,-rpath," + _build.LIBDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    got = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.decode().splitlines()}
    hexes = lambda name: [float.fromhex(t) for t in got[name]]      # noqa: E731
    n1, k = 19, 3
    ublock, iblock, (umap, imap, plain, y), (tumap, timap, tplain, ty) = cpp_problem()
    users, items = fmhip.Relation(ublock, umap), fmhip.Relation(iblock, imap)
    rd = fmhip.RelationalData(y, [users, items], plain=fmhip.DataSet(*plain, y, batch_rows=0)).cache()
    rt = fmhip.RelationalData(ty, [users.remap(tumap), items.remap(timap)], plain=fmhip.DataSet(*tplain, ty, batch_rows=0)).cache()
    fm = fmhip.FMModel(n1 - 1, k)
    fm.w0, fm.w = 0.1, np.array([0.02 * ((i % 7) - 3) for i in range(n1)])
    fm.v = np.array([[0.01 * ((f * 7 + i * 3) % 11 - 5) for i in range(n1)] for f in range(k)])
    mcmc = fmhip.HipBlockMCMC.run(seed=12, groups="parts", test=rt)
    for _ in range(3):
        mcmc.learn(fm, rd)
    st = mcmc.state
    assert hexes("w0") == [fm.w0] and hexes("w") == fm.w.tolist() and hexes("v") == fm.v.reshape(-1, order="F").tolist()
    assert hexes("alpha") == [st["alpha"]] and hexes("lambda") == st["lambda"].reshape(-1).tolist() and hexes("mu") == st["mu"].reshape(-1).tolist()
    assert hexes("mean") == mcmc.predictions().tolist()
    assert [int(c) for c in got["counts"]] == mcmc.group_counts.tolist() and got["groups"] == ["3"]
