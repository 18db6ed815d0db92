"""Every training rule on every dataset layout: AdaGrad (with and without decay), FTRL-Proximal, weighted single rows under SGD and
AdaGrad and weighted pairs, each under both losses, on the named layouts of layout_cases.py — the dense hot block's page 0 and
gradient-side pages, a hot row with an exactly zero gradient, the rows-only update driven by hot ids, a named single-batch hot block,
row-blocked transposes, the flat-address kernels.  The twins are the existing ones (train_ref, ftrl_ref, weight_ref); the tolerances
are imported from the rules' own files (test_gpu_adagrad.check_step, test_gpu_ftrl.check_step / check_epochs,
test_gpu_weights.check_step; rel-L2 1e-5 for trajectories), never restated.

The covering table (layout_cases.CASES; `rule k` + the loss's initial — s: squared, l: logistic).  Every rule meets every layout;
every k of 8 / 32 / 64 / 100 meets page0, pages, absent and wide under each update rule (SGD: w_sgd, w_pairs; AdaGrad:
adagrad_decay, adagrad, w_adagrad; FTRL); one case runs at k = 256:
    page0         ftrl 8s, ftrl 32l, ftrl 64s, ftrl 100l, w_sgd 8s, w_pairs 32l, w_sgd 64s, w_pairs 100l, adagrad_decay 8s, adagrad 32l, w_adagrad 64s, adagrad 100l
    pages         ftrl 8l, ftrl 32s, ftrl 64l, ftrl 100s, w_sgd 32l, w_pairs 64s, w_sgd 100l, w_pairs 8s, adagrad_decay 32l, adagrad 64s, w_adagrad 100l, adagrad_decay 8s, adagrad 256s
    absent        ftrl 8s, ftrl 32l, ftrl 64s, ftrl 100l, w_sgd 64s, w_pairs 100l, w_sgd 8s, w_pairs 32l, adagrad_decay 64s, adagrad 100l, w_adagrad 8s, w_adagrad 32l
    wide          ftrl 8l, ftrl 32s, ftrl 64l, ftrl 100s, w_sgd 100l, w_pairs 8s, w_sgd 32l, w_pairs 64s, adagrad_decay 100l, adagrad 8s, w_adagrad 32l, adagrad 64s
    all_hot_wide  adagrad_decay 8s, adagrad 32l, ftrl 64s, w_sgd 100l, w_adagrad 8s, w_pairs 32l
    named_single  adagrad_decay 32l, adagrad 64s, ftrl 100l, w_sgd 8s, w_adagrad 32l, w_pairs 64s
    row_blocked   adagrad_decay 64s, adagrad 100l, ftrl 8s, w_sgd 32l, w_adagrad 64s, w_pairs 100l
    flat_page0    adagrad_decay 100l, adagrad 8s, ftrl 32l, w_sgd 64s, w_adagrad 100l, w_pairs 8s
    flat_wide     adagrad_decay 8s, adagrad 32l, ftrl 64s, w_sgd 100l, w_adagrad 8s, w_pairs 32l
(test_host_layout_cases.py holds this text to the table, the table to its promises, every layout to its claims and the FTRL caps to
the twin alone.)

Every one-step comparison also runs on the same rows built with hot_block=False, held to the same tolerance (the control): a
failure of both is a hot row's sum cancelling beyond fp32 — another seed, noted in layout_cases.SEEDS; a failure of the hot layout
alone is a finding."""
import numpy as np
import pytest

import ftrl_ref as fref
import layout_cases as lc
import test_gpu_adagrad as tada
import test_gpu_ftrl as tftrl
import test_gpu_weights as twts
import train_ref as ref
import weight_ref as wref
from train_ref import rel, same

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fmhip():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import sparkfm_amd
    return sparkfm_amd


def L():
    from sparkfm_amd import _ffi
    return _ffi.load()


def f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def dataset(fmhip, case, hot=True, y=None):
    """The case's rows as a cached DataSet: built as the layout says, or (hot=False) with the hot block off."""
    a, build = case.lay.a, case.lay.build if hot else lc.build_without_hot_block(case.lay)
    return fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"] if y is None else y, weights=case.c, **build).cache()


def model(fmhip, case, tune=None):
    """A model at the case's parameters, set to its loss (flat layouts: on the flat-address kernels), with `tune` applied."""
    from sparkfm_amd import _ffi
    a = case.lay.a
    fm = fmhip.FMModel(a["n1"] - 1, a["k"])
    fm.w0, fm.w, fm.v = a["w0"], a["w"], a["v"]
    _ffi.check(L().fmhip_model_set_loss(fm.handle, _ffi.loss_code(case.loss)))
    for key, val in dict({"FLAT_ADDRESS": 1} if case.lay.flat else {}, **(tune or {})).items():
        _ffi.check(L().fmhip_model_tune(fm.handle, _ffi.TUNE[key], val))
    return fm


def learner(fmhip, case, shuffle_seed=None, l1=None):
    """The case's learner (l1: in place of the one-step L1 pair of an FTRL case)."""
    if case.rule == "ftrl":
        l1 = case.l1 if l1 is None else l1
        return fmhip.HipFTRL(alpha=lc.ETA, beta=fref.BETA, l1w=l1[0], l1v=l1[1], l2_0=case.regs[0], l2w=case.regs[1], l2v=case.regs[2],
                             ftrl_init=fref.INIT, loss=case.loss, shuffle_seed=shuffle_seed)
    return fmhip.HipSGD(eta=lc.ETA, reg0=case.regs[0], regw=case.regs[1], regv=case.regs[2], loss=case.loss, optimizer=case.update if case.update != "ftrl" else "sgd",
                        adagrad_eps=lc.EPS, adagrad_init=lc.INIT, pairs=case.pairs, shuffle_seed=shuffle_seed)


def state(fm, case):
    """Parameters and the rule's state as the device holds them (before the first step a model hands back the fp64 values it was
    given: rounded to fp32 here, which is the identity on what the device wrote)."""
    out = (float(f32(fm.w0)), f32(fm.w), f32(fm.v))
    if case.update == "ftrl":
        st = fm.ftrl_state()
        return out + tuple(st[n] for n in tftrl.STATE)
    return out + (tada.get_state(fm) if case.update == "adagrad" else ())


def put_rule(fm, case):
    """The case's update rule on the model (what learner.step does first), so that its state can be read before a step."""
    if case.update == "ftrl":
        tftrl.set_ftrl(fm, fref.BETA, fref.INIT, *case.l1)
    elif case.update == "adagrad":
        tada.set_opt(fm, eps=lc.EPS, init=lc.INIT)


def check_one_step(fm, case, s0, s1):
    """The rule's own one-step comparison, imported."""
    if case.update == "ftrl":
        tftrl.check_step(fm, s0, s1, lc.ETA, case.twin_rule)
    elif case.update == "adagrad":
        tada.check_step(fm, s0, s1, lc.INIT, lc.ETA)
    else:
        twts.check_step(fm, s0, s1)


def assert_layout(ds, lay, hot=True):
    """ds.layout() reports what the layout promised (hot=False: no hot block at all); on the wide layouts every batch passes
    step_apply's few_rows test, counted from batch_info's n_columns."""
    got, a = ds.layout(), lay.a
    if not hot:
        assert got["hot_pages"] == 0 and got["hot_ids_all"] == [] and got["nnz_sparse"] == got["nnz_sparse_backward"] == len(a["col"])
        return
    assert sorted(got["hot_ids"]) == lay.hot_ids and sorted(got["hot_ids_all"]) == lay.hot_ids_all and got["hot_pages"] == lay.hot_pages
    assert got["nnz_sparse"] == int((~np.isin(a["col"], lay.hot_ids)).sum())
    assert got["nnz_sparse_backward"] == int((~np.isin(a["col"], lay.hot_ids_all)).sum())
    bs = lc.batches(lay)
    assert ds.n_batches == len(bs)
    if lay.name in lc.ROWS_ONLY_LAYOUTS:
        for b, (r0, r1) in enumerate(bs):
            present = np.unique(a["col"][a["row_ptr"][r0]:a["row_ptr"][r1]])
            n_cold = ds.batch_info(b)["n_columns"] - int(np.isin(present, lay.hot_ids_all).sum())
            assert n_cold == len(lc.cold_columns(lay, b)) and 2 * (n_cold + lc.HOT_T * got["hot_pages"]) <= a["n1"], b


def check_epochs(fm, case, s, hot):
    """The rules' trajectory bounds (test_gpu_ftrl.check_epochs; rel-L2 1e-5 of test_gpu_adagrad.test_epochs_vs_reference and
    test_gpu_weights.test_epochs_vs_twin), and the same bound over the hot rows ALONE: sixteen wrong rows must not hide."""
    got = dict(v=fm.v, w=fm.w)
    if case.update == "ftrl":
        tftrl.check_epochs(fm, s)
        st = fm.ftrl_state()
        got.update(zv=st["zv"], zw=st["zw"], nv=st["nv"], nw=st["nw"])
    else:
        if case.update == "adagrad":
            n0, nw, nv = tada.get_state(fm)
            got.update(nv=nv, nw=nw)
            assert n0 == pytest.approx(s.n0, rel=1e-5)
        errs = {n: rel(x, getattr(s, n)) for n, x in got.items()}
        print(errs)
        assert max(errs.values()) <= 1e-5, errs
        assert fm.w0 == pytest.approx(s.w0, rel=1e-5, abs=1e-6)
    hot_errs = {n: rel(x[..., hot], getattr(s, n)[..., hot]) for n, x in got.items()}
    print("hot rows:", hot_errs)
    assert max(hot_errs.values()) <= 1e-5, hot_errs


# ---- 1. every case of the table: the layout, one step of every batch (with its control), three shuffled epochs -----------------

@pytest.mark.parametrize("rule,name,k,loss", lc.CASES, ids=["%s-%s-%d-%s" % c for c in lc.CASES])
def test_rule_on_layout(fmhip, rule, name, k, loss):
    case = lc.Case(rule, name, k, loss)
    lay, lrn = case.lay, learner(fmhip, case)
    ds, ctl = dataset(fmhip, case), dataset(fmhip, case, hot=False)
    assert_layout(ds, lay)
    assert_layout(ctl, lay, hot=False)
    if case.c is not None:
        assert ds.deviceWeights()["weighted"] and (case.c == 0).any()
    s0 = case.start()
    for b, (r0, r1) in enumerate(lc.batches(lay)):
        s1 = case.step(s0.copy(), r0, r1)
        for which, data in (("control", ctl), ("hot", ds)):
            fm = model(fmhip, case)
            st = lrn.step(fm, data, b)
            assert st["rows"] == r1 - r0 and st["nonfinite"] == 0
            try:
                check_one_step(fm, case, s0, s1)
            except AssertionError as e:
                why = ("the control (hot block off) misses the tolerance too: a sum cancelling beyond fp32, pick another seed" if which == "control"
                       else "the hot layout ALONE misses the tolerance its control meets")
                raise AssertionError("batch %d, %s: %s" % (b, why, e))
            fm.close()
    ctl.unpersist()
    # three shuffled epochs (FTRL: under the epochs' L1, layout_cases.Case says why)
    fm, lrn = model(fmhip, case), learner(fmhip, case, shuffle_seed=3, l1=getattr(case, "l1_epochs", None))
    orders = []
    for _ in range(3):
        orders.append(lrn.batch_order(ds.n_batches).tolist())
        lrn.learn(fm, ds)
    assert orders == lc.shuffled_orders(3, ds.n_batches, 3)
    s = case.epochs(case.start(), orders)
    check_epochs(fm, case, s, lay.hot_ids_all)
    if rule == "ftrl":
        assert (s.v == 0).any() and (s.w == 0).any() and (s.v != 0).any() and (s.w != 0).any()
    assert np.abs(fm.v - f32(lay.a["v"])).max() > 1e-4            # it moved
    ds.unpersist()
    fm.close()


# ---- 2. bit-level properties, GPU against GPU -------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [8, 32, 100])
@pytest.mark.parametrize("rule", ["ftrl", "adagrad"])
@pytest.mark.parametrize("name", ["wide", "all_hot_wide"])
def test_rows_only_equals_dense_bitwise_on_a_hot_block(fmhip, name, rule, k):
    """Every batch in turn through fmhip_sgd_step (its update: k_apply_rows over the batch's columns AND the hot block's ids) and
    through fmhip_step_compute + fmhip_step_apply (k_apply over the whole model), FTRL with L1 and L2 on / AdaGrad without decay:
    theta, n and zeta equal bit for bit (test_gpu_ftrl.test_rows_only_equals_dense_bitwise without a hot block), the hot rows moved,
    and the rows no batch touched keep the bits of the start."""
    from sparkfm_amd import _ffi
    case = lc.Case(rule, name, k, "logistic")
    outs = []
    for dense in (False, True):
        ds, fm = dataset(fmhip, case), model(fmhip, case)
        assert_layout(ds, case.lay)
        put_rule(fm, case)
        start = state(fm, case)
        for b in range(ds.n_batches):
            if dense:
                _ffi.check(L().fmhip_step_compute(fm.handle, ds.handle, b))
                _ffi.check(L().fmhip_step_apply(fm.handle, lc.ETA, *case.regs))
            else:
                _ffi.check(L().fmhip_sgd_step(fm.handle, ds.handle, b, lc.ETA, *case.regs, None))
        fm._device_updated()
        outs.append(state(fm, case))
        ds.unpersist()
        fm.close()
    assert same(outs[0], outs[1])
    hot, untouched = case.lay.hot_ids_all, np.setdiff1d(np.arange(case.lay.a["n1"]), case.lay.a["col"])
    assert len(untouched) > case.lay.a["n1"] // 2
    for got, was in zip(outs[0][1:], start[1:]):
        if np.ndim(got) == 0:
            continue
        assert np.array_equal(got[..., untouched], was[..., untouched])
        moved = got[..., hot] != was[..., hot]
        assert (moved if np.ndim(got) == 1 else moved.any(axis=0)).all()          # every hot row took its update


@pytest.mark.parametrize("k", [8, 32, 100])
@pytest.mark.parametrize("rule", ["ftrl", "ftrl_plain", "adagrad"])
def test_an_absent_hot_row_keeps_its_bits(fmhip, rule, k):
    """The `absent` layout: after the step of batch 1 (two hot features in none of its rows; the dense update) and of the last batch
    (one; 12 rows of 500 features: the rows-only update, which LISTS the hot ids), the absent feature's theta row, w entry, accumulator
    and zeta are bit-equal to before the step — under FTRL with L1 and L2 on, FTRL with neither, and AdaGrad without decay.  The block
    product gives a column of zeros an exactly zero gradient, and a zero gradient moves nothing under these rules (fm_apply.hip)."""
    case = lc.Case("ftrl" if rule.startswith("ftrl") else rule, "absent", k, "squared")
    if rule == "ftrl_plain":
        case.regs, case.l1 = (0.0, 0.0, 0.0), (0.0, 0.0)
    ds, lrn = dataset(fmhip, case), learner(fmhip, case)
    assert_layout(ds, case.lay)
    assert lc.few_rows(case.lay, 4) and not lc.few_rows(case.lay, 1)
    for b, ids in sorted(case.lay.absent.items()):
        fm = model(fmhip, case)
        put_rule(fm, case)
        before = state(fm, case)
        lrn.step(fm, ds, b)
        after = state(fm, case)
        present = np.setdiff1d(case.lay.hot_ids_all, ids)
        for got, was in zip(after[1:], before[1:]):
            if np.ndim(got) == 0:
                continue
            assert np.array_equal(got[..., ids], was[..., ids]), (b, ids)
            assert not np.array_equal(got[..., present], was[..., present])
        fm.close()
    ds.unpersist()


@pytest.mark.parametrize("k", [8, 32])
def test_an_absent_hot_row_decays_once_under_lazy_sgd(fmhip, k):
    """Plain SGD with decay on the `absent` layout's last batch (the rows-only update with lazy decay): the absent hot feature's row,
    read back through fm.v, is its start times (1 - eta regv) — the stored row times the new scale equals the eager decay
    (test_rows_only_update_when_every_feature_sits_in_the_hot_block's read-back and tolerance)."""
    case = lc.Case("adagrad_decay", "absent", k, "squared")
    a, (b, ids) = case.lay.a, sorted(case.lay.absent.items())[-1]
    ds, fm = dataset(fmhip, case), model(fmhip, case)
    assert_layout(ds, case.lay)
    assert lc.few_rows(case.lay, b)
    fmhip.HipSGD(eta=lc.ETA, reg0=lc.REGS[0], regw=lc.REGS[1], regv=lc.REGS[2]).step(fm, ds, b)
    np.testing.assert_allclose(fm.v[:, ids], a["v"][:, ids] * (1 - lc.ETA * lc.REGS[2]), rtol=2e-6)
    np.testing.assert_allclose(fm.w[ids], a["w"][ids] * (1 - lc.ETA * lc.REGS[1]), rtol=2e-6)
    present = np.setdiff1d(case.lay.hot_ids_all, ids)
    assert (np.abs(fm.v[:, present] - a["v"][:, present] * (1 - lc.ETA * lc.REGS[2])) > 1e-6).any(axis=0).all()
    ds.unpersist()
    fm.close()


@pytest.mark.parametrize("rule", ["ftrl", "adagrad_decay", "adagrad"])
@pytest.mark.parametrize("name", ["page0", "wide"])
def test_switches_change_no_bit_on_a_hot_block(fmhip, name, rule):
    """One epoch at k = 32: FMHIP_TUNE_FUSED_UPDATE = 1, FMHIP_TUNE_MERGED_FINISH = 0 / 1 and FMHIP_TUNE_BACKWARD_KERNEL = 0 only choose
    where and how an SGD step's pieces run; under AdaGrad and FTRL the results keep every bit, and two runs are bit-identical."""
    case = lc.Case(rule, name, 32, "logistic")
    ds = dataset(fmhip, case)
    assert_layout(ds, case.lay)
    outs = []
    for tune in ({}, {}, {"FUSED_UPDATE": 1}, {"MERGED_FINISH": 0}, {"MERGED_FINISH": 1}, {"BACKWARD_KERNEL": 0}):
        fm = model(fmhip, case, tune)
        learner(fmhip, case).learn(fm, ds)
        outs.append(state(fm, case))
        fm.close()
        assert same(outs[0], outs[-1]), tune
    assert np.abs(outs[0][2] - f32(case.lay.a["v"])).max() > 1e-4
    ds.unpersist()


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k", [8, 32])
def test_labels_of_zero_weight_rows_change_no_bit_on_a_hot_block(fmhip, k, loss):
    """test_gpu_weights.test_labels_of_zero_weight_rows_change_no_bit on the page0 layout: the q-mode forward with the hot prologue,
    the weights' finish, the block product reading P and e — a zero-weight row's residual is +0 whatever its label."""
    case = lc.Case("w_sgd", "page0", k, loss)
    zero = case.c == 0
    assert 100 < zero.sum() < 400
    y2 = case.lay.a["y"].copy()
    y2[zero] = np.where(y2[zero] > 0, -50.0, 77.0)
    outs = []
    for y in (case.lay.a["y"], y2):
        ds, fm, lrn = dataset(fmhip, case, y=y), model(fmhip, case), learner(fmhip, case)
        assert_layout(ds, case.lay)
        stats = [lrn.step(fm, ds, b) for b in range(ds.n_batches)]
        outs.append(state(fm, case) + tuple(s["sse"] for s in stats) + tuple(s["sum_e"] for s in stats))
        ds.unpersist()
        fm.close()
    assert same(outs[0], outs[1])
    assert np.abs(outs[0][2] - f32(case.lay.a["v"])).max() > 1e-4


# ---- 3. data-parallel, two thread ranks in one process ---------------------------------------------------------------------------

def shards_of(a, cuts, c=None):
    """The problem's rows split at `cuts` into one shard per rank (c: the rows' weights, split alike)."""
    out = []
    for r0, r1 in zip([0] + cuts, cuts + [len(a["y"])]):
        p0, p1 = int(a["row_ptr"][r0]), int(a["row_ptr"][r1])
        d = dict(row_ptr=a["row_ptr"][r0:r1 + 1] - p0, col=a["col"][p0:p1], val=a["val"][p0:p1], y=a["y"][r0:r1])
        out.append(d if c is None else dict(d, weights=c[r0:r1]))
    return out


@pytest.mark.parametrize("rule,exchange", [("ftrl", "touched"), ("adagrad", "touched"), ("w_sgd", "dense")])
def test_data_parallel_on_hot_shards(fmhip, rule, exchange):
    """World 2, thread ranks: the page0 rows split 900 / 300 (rank 0: four batches of 297, 297, 297 and 9 rows with page 0 asserted;
    rank 1: 297 and 3), k = 32, two epochs.  touched: FTRL (L1 and L2 on) and AdaGrad without decay on a model eight times wider than
    the data — the compact gradient with the hot block's positions; dense: weighted logistic SGD.  Replicas bit-equal; the twins'
    dp_epochs matched at rel-L2 1e-5, and over the hot rows alone."""
    from sparkfm_amd import DataSet, FMModel
    from sparkfm_amd.distributed import HipDataParallelFTRL, HipDataParallelSGD, ThreadStagedComm, run_thread_ranks
    k, br, n_epochs = 32, 297, 2
    loss = "logistic" if rule == "w_sgd" else "squared"
    case = lc.Case(rule, "page0", k, loss)
    lay, n1 = case.lay, 4003 if exchange == "touched" else 503
    shards = shards_of(lay.a, [900], case.c)
    want0 = lc.expected_layout(dict(shards[0], n1=lay.a["n1"]), dict(batch_rows=br))
    assert want0["hot_pages"] == 1 and want0["hot_ids"] == lay.hot_ids
    regs = fref.L2 if rule == "ftrl" else ((0.0, 0.0, 0.0) if rule == "adagrad" else (0.0, 1e-3, 1e-3))

    def rank_fn(r, group):
        ds = DataSet.from_arrays(shards[r], batch_rows=br, device=0).cache()
        got = ds.layout()
        fm = FMModel(n1 - 1, k, device=0)
        fm.w0, fm.w, fm.v = ref.dp_init(n1, k)
        comm = ThreadStagedComm(fm, r, group)
        kw = dict(exchange=exchange, upper_fractions=ref.DP_FRACTIONS[exchange], loss=loss)
        if rule == "ftrl":
            dp = HipDataParallelFTRL(comm, alpha=lc.ETA, beta=fref.BETA, l1w=tftrl.DP_L1[0], l1v=tftrl.DP_L1[1], l2_0=regs[0], l2w=regs[1], l2v=regs[2],
                                     ftrl_init=fref.INIT, **kw)
        else:
            dp = HipDataParallelSGD(comm, eta=lc.ETA, reg0=regs[0], regw=regs[1], regv=regs[2], optimizer=case.update, adagrad_eps=lc.EPS,
                                    adagrad_init=lc.INIT, **kw)
        out = {}
        try:
            dp.plan(fm, ds)
            for _ in range(n_epochs):
                dp.learn(fm, ds)
            out = dict(bits=state(fm, case), rc=0, layout=got, n_batches=ds.n_batches)
        except Exception as ex:           # noqa: BLE001 — reported by the assertion below
            out = dict(rc=getattr(ex, "code", "?"), msg=str(ex))
        group.barrier()
        comm.close()
        ds.unpersist()
        fm.close(discard=True)
        return out

    res = run_thread_ranks(2, rank_fn, timeout=300.0)
    assert all(o["rc"] == 0 for o in res), [o.get("msg") for o in res]
    assert res[0]["n_batches"] == 4 and res[0]["layout"]["hot_pages"] == 1 and sorted(res[0]["layout"]["hot_ids"]) == lay.hot_ids
    assert same(res[0]["bits"], res[1]["bits"])
    w0, w, v = ref.dp_init(n1, k)
    if rule == "ftrl":
        s = fref.dp_epochs(fref.State(w0, w, v, fref.INIT, fref.BETA), shards, br, [None] * n_epochs, lc.ETA, *regs,
                           fref.Rule(loss, False, fref.BETA, *tftrl.DP_L1))
        names = ("w0", "w", "v") + tftrl.STATE
    elif rule == "adagrad":
        s = ref.dp_epochs(ref.State(w0, w, v, lc.INIT), shards, br, [None] * n_epochs, lc.ETA, *regs, ref.Rule(loss, False, lc.EPS))
        names = ("w0", "w", "v", "n0", "nw", "nv")
    else:
        s = wref.dp_epochs(wref.State(w0, w, v), shards, br, [None] * n_epochs, lc.ETA, *regs, wref.Rule(loss, False, None))
        names = ("w0", "w", "v")
    got = dict(zip(names, res[0]["bits"]))
    hot = lay.hot_ids_all
    errs = {n: rel(got[n], getattr(s, n)) for n in names if np.ndim(got[n])}
    hot_errs = {n: rel(got[n][..., hot], getattr(s, n)[..., hot]) for n in names if np.ndim(got[n])}
    print(errs, "hot rows:", hot_errs)
    assert max(errs.values()) <= 1e-5 and max(hot_errs.values()) <= 1e-5, (errs, hot_errs)
    assert abs(got["w0"] - s.w0) <= 1e-5 * abs(s.w0) + 1e-6
    assert np.abs(got["v"][:, hot] - f32(v)[:, hot]).max() > 1e-4
    if exchange == "touched":       # the rows no rank ever touched hold their first bits
        assert np.array_equal(got["v"][:, 500:], f32(v)[:, 500:])


# ---- 4. the random-shapes property under the rules ---------------------------------------------------------------------------------

RANDOM_SEED = 20261021
RANDOM_L1 = (0.1, 0.01)


def random_case(rng, seed, case, rule):
    """One case of test_gpu_parity._random_shapes's generator within rows <= 600 and n1 <= 3000: the problem, batch_rows, whether the
    hot block is on, the regularisers.  FTRL: rows of at least two entries (ftrl_ref.one_step_problem says why)."""
    from helpers import random_problem
    k = int(rng.choice([1, 2, 5, 8, 13, 16, 32, 40, 64, 100]))
    n_rows = int(rng.integers(2, 601))
    n1 = int(rng.integers(3, 400)) if case < 14 else int(rng.integers(400, 3001))     # wide models: the rows-only update
    hi = int(rng.integers(2, min(n1, 40) + 1))
    lo = int(rng.integers(2 if rule == "ftrl" else 0, hi + 1))
    batch_rows = int(rng.choice([0, 7, 64, 300]))
    empty = () if rule == "ftrl" else tuple(rng.integers(0, n_rows, 2).tolist())
    a = random_problem(seed * 1000 + case, n_rows, n1, k, lo, hi, empty_rows=empty)
    a["val"] = a["val"].astype(np.float32).astype(np.float64)
    if case % 3 == 0 and len(a["col"]):                              # two dominating features
        hot = rng.integers(0, n1, 2)
        for r in range(n_rows):
            s = slice(a["row_ptr"][r], a["row_ptr"][r + 1])
            if s.stop - s.start >= 2 and not np.isin(hot, a["col"][s]).any():
                a["col"][s.start] = hot[0]
    if rule == "w_sgd":
        a["y"] = (rng.random(n_rows) < 0.4).astype(np.float64)
    decay = case % 4 != 0 if rule != "w_sgd" else case % 2 == 0      # AdaGrad: decay on in three quarters of the cases
    return a, batch_rows, case % 5 != 4, (0.01, 0.01, 0.01) if decay or rule == "ftrl" else (0.0, 0.0, 0.0)


def random_twin(a, rule, br, eta, regs, c, dtype=np.float64):
    """-> the twin after one epoch of ascending batches, or None where the oracle diverged.  dtype (FTRL): ftrl_ref's fp32 run."""
    with np.errstate(all="ignore"):
        if rule == "ftrl":
            s = fref.epochs(fref.State(a["w0"], a["w"], a["v"], fref.INIT, fref.BETA, dtype), a, br, [None], eta, *regs,
                            fref.Rule("squared", False, fref.BETA, *RANDOM_L1))
        elif rule == "adagrad":
            s = ref.epochs(ref.State(a["w0"], a["w"], a["v"], lc.INIT), a, br, [None], eta, *regs, ref.Rule("squared", False, lc.EPS))
        else:
            s = wref.epochs(wref.State(a["w0"], a["w"], a["v"]), a, c, br, [None], eta, *regs, wref.Rule("logistic", False, None))
    return s if np.isfinite(s.v).all() and np.abs(s.v).max() < 1e3 and np.isfinite(s.w).all() else None


def random_cases(rule, seed, cases):
    """Yields (case, problem, batch_rows, rows per batch, hot block on?, regularisers, eta, weights or None)."""
    rng = np.random.default_rng(seed)
    for case in range(cases):
        a, batch_rows, hot, regs = random_case(rng, seed, case, rule)
        n_rows = len(a["y"])
        br = n_rows if batch_rows <= 0 or batch_rows > n_rows else batch_rows
        eta = 0.02 if br >= 64 else 0.001                            # _random_shapes's step sizes
        yield case, a, batch_rows, br, hot, regs, eta, wref.draw_weights(seed + case, n_rows) if rule == "w_sgd" else None


def random_shapes_under_rule(fmhip, rule, seed=RANDOM_SEED, cases=24, max_dropped=2):
    dropped = 0
    for case, a, batch_rows, br, hot, regs, eta, c in random_cases(rule, seed, cases):
        n_rows = len(a["y"])
        s = random_twin(a, rule, br, eta, regs, c)
        if s is None:                                                # only a diverged oracle drops a case
            dropped += 1
            continue
        ds = fmhip.DataSet(a["row_ptr"], a["col"], a["val"], a["y"], batch_rows=batch_rows, hot_block=None if hot else False, weights=c).cache()
        fm = fmhip.FMModel(a["n1"] - 1, a["k"])
        fm.w0, fm.w, fm.v = a["w0"], a["w"], a["v"]
        if rule == "ftrl":
            lrn = fmhip.HipFTRL(alpha=eta, beta=fref.BETA, l1w=RANDOM_L1[0], l1v=RANDOM_L1[1], l2_0=regs[0], l2w=regs[1], l2v=regs[2], ftrl_init=fref.INIT)
        elif rule == "adagrad":
            lrn = fmhip.HipSGD(eta=eta, reg0=regs[0], regw=regs[1], regv=regs[2], optimizer="adagrad", adagrad_eps=lc.EPS, adagrad_init=lc.INIT)
        else:
            lrn = fmhip.HipSGD(eta=eta, reg0=regs[0], regw=regs[1], regv=regs[2], loss="logistic")
        lrn.learn(fm, ds)
        what = (rule, seed, case, a["k"], n_rows, a["n1"], batch_rows, hot, ds.layout()["hot_pages"])
        # _random_shapes's epoch bound
        assert np.linalg.norm(fm.v - s.v) <= 1e-5 * max(np.linalg.norm(s.v), 1e-9), what
        assert np.linalg.norm(fm.w - s.w) <= 1e-5 * max(np.linalg.norm(s.w), 1e-9), what
        assert fm.w0 == pytest.approx(float(s.w0), rel=1e-5, abs=1e-6), what
        ds.unpersist()
        fm.close()
    assert dropped <= max_dropped, (rule, seed, dropped)
    return dropped


@pytest.mark.parametrize("rule", ["adagrad", "ftrl", "w_sgd"])
def test_random_shapes_under_rules(fmhip, rule):
    """test_gpu_parity's random-shapes property under the newer rules: 24 cases per rule (rows <= 600, n1 <= 3000, a third with two
    dominating features, a fifth with the hot block off, batch sizes from 0 / 7 / 64 / 300), one epoch under AdaGrad (decay on in three
    quarters of the cases), FTRL with L1 and L2 on, and weighted logistic SGD, against the matching twin at _random_shapes's own epoch
    bound.  Only a diverged oracle drops a case, in at most 2 of the 24 (none at this seed, as counted on the CPU).
    tools/soak_random_shapes.py runs it over more seeds."""
    random_shapes_under_rule(fmhip, rule)
