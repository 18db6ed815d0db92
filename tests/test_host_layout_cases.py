"""layout_cases.py on the CPU: every named layout is what it claims (recomputed in numpy from the library's rule), the covering table
of test_gpu_rules_by_layout.py covers what it says, and the fp64 twin ALONE meets the caps the GPU tests rely on (FTRL's share of
zeros and its near-threshold cap, check_step's "it moved by AdaGrad's steps") at the seeds layout_cases.py holds."""
import numpy as np
import pytest

import ftrl_ref as fref
import layout_cases as lc


@pytest.fixture(scope="module", params=[(n, p) for n in lc.NAMES for p in (False, True)], ids=lambda x: x[0] + ("-pairs" if x[1] else ""))
def lay(request):
    return lc.layout(request.param[0], 8, pairs=request.param[1])


def row_share(a, ids, r0=0, r1=None):
    """The share of the rows [r0, r1) that hold each of `ids`."""
    r1 = len(a["y"]) if r1 is None else r1
    c = a["col"][a["row_ptr"][r0]:a["row_ptr"][r1]]
    return np.bincount(c, minlength=a["n1"])[ids] / float(r1 - r0)


def test_the_layout_is_what_it_claims(lay):
    a = lay.a
    n_rows = len(a["y"])
    assert n_rows <= 1500 and a["n1"] <= 6000
    want = lc.expected_layout(a, lay.build)
    assert (want["hot_ids"], want["hot_ids_all"], want["hot_pages"]) == (lay.hot_ids, lay.hot_ids_all, lay.hot_pages)
    assert lc.expected_layout(a, lc.build_without_hot_block(lay))["hot_pages"] == 0
    # frequencies: page 0 at >= 10 % of the rows, the gradient-side pages in the 5-10 % band
    rest = sorted(set(lay.hot_ids_all) - set(lay.hot_ids))
    assert (row_share(a, lay.hot_ids) >= 0.10).all() and 2 <= len(lay.hot_ids) <= 16
    if rest:
        share = row_share(a, rest)
        if len(lay.hot_ids) == 16:        # a full page 0: the next most frequent features follow, whatever their share
            assert share.max() <= row_share(a, lay.hot_ids).min()
        else:
            assert (share >= 0.05).all() and (share < 0.10).all()
    # no hot id twice in a row or with a stored zero (fp32, as the library reads the values)
    rows = np.repeat(np.arange(n_rows), np.diff(a["row_ptr"]))
    hot = np.isin(a["col"], lay.hot_ids_all)
    key = rows[hot].astype(np.int64) * a["n1"] + a["col"][hot]
    assert len(np.unique(key)) == len(key)
    assert (a["val"][hot].astype(np.float32) != 0).all()
    assert len(fref.cancelling_features(a["row_ptr"], a["col"], a["n1"])) == 0


def test_batches_are_what_the_table_says(lay):
    bs = lc.batches(lay)
    base = lay.name[5:] if lay.flat else lay.name
    if base in ("page0", "absent", "row_blocked"):
        assert len(bs) == 5 and all((r1 - r0) % 16 and (r1 - r0) % 64 for r0, r1 in bs[:4]) and bs[4][1] - bs[4][0] in (12, 8)
    if base == "named_single":
        assert len(bs) == 1 and lay.build["hot_block"] == 4
    if base in lc.ROWS_ONLY_LAYOUTS or lay.name in lc.ROWS_ONLY_LAYOUTS:
        assert all(lc.few_rows(lay, b) for b in range(len(bs)))           # 2 * (cold columns + 16 * pages) <= n1
    if base == "all_hot_wide":
        assert all(len(lc.cold_columns(lay, b)) == 0 for b in range(len(bs)))
    if base == "pages":
        assert lay.hot_pages == 3 and len(lay.hot_ids) == 15 and len(lay.hot_ids_all) == 40
    assert all((r1 - r0) % 2 == 0 for r0, r1 in bs) or lay.build["batch_rows"] == 297


def test_absent_features_are_absent(lay):
    if not lay.name.endswith("absent"):
        assert lay.absent == {}
        return
    bs = lc.batches(lay)
    assert sorted(lay.absent) == [1, 4] and len(lay.absent[1]) == 2 and len(lay.absent[4]) == 1
    for b, ids in lay.absent.items():
        assert (row_share(lay.a, ids, *bs[b]) == 0).all()
        for other in range(len(bs)):
            if other not in lay.absent:
                assert (row_share(lay.a, ids, *bs[other]) > 0).all()
        assert (row_share(lay.a, ids) >= 0.10).all() and set(ids) <= set(lay.hot_ids)


def test_the_table_covers_what_it_says():
    cases = lc.CASES
    assert len(set(cases)) == len(cases)
    for rule in lc.RULES:
        assert {n for r, n, k, l in cases if r == rule} == set(lc.NAMES), rule
        assert {l for r, n, k, l in cases if r == rule} == set(lc.LOSSES), rule
    for upd in ("sgd", "adagrad", "ftrl"):
        for name in lc.MAIN:
            assert {k for r, n, k, l in cases if lc.UPDATE_RULE[r] == upd and n == name} >= set(lc.KS), (upd, name)
    assert sum(k == 256 for r, n, k, l in cases) == 1
    import test_gpu_rules_by_layout as t
    assert lc.table() in t.__doc__


@pytest.mark.parametrize("rule,name,k,loss", [c for c in lc.CASES if c[0] == "ftrl"], ids=lambda x: str(x))
def test_ftrl_caps_hold_for_the_twin_alone(rule, name, k, loss):
    """What test_gpu_ftrl.check_step asserts of the twin's own numbers, for every batch's step from the start: 30-70 % of the touched
    coordinates on zero, at most ZERO_CAP of them within tolerance of the L1 threshold."""
    case = lc.Case(rule, name, k, loss)
    s0 = case.start()
    for r0, r1 in lc.batches(case.lay):
        s1 = case.step(s0.copy(), r0, r1)
        near = fref.near_threshold(s0, s1, lc.ETA, case.twin_rule)
        for p, g in (("w", s1.g[1]), ("v", s1.g[2])):
            touched = g != 0
            share = ((getattr(s1, p) == 0) & touched).sum() / max(touched.sum(), 1)
            assert 0.3 <= share <= 0.7, (p, r0, share)
            assert near[p].sum() <= fref.ZERO_CAP * touched.sum(), (p, r0, int(near[p].sum()), int(touched.sum()))


@pytest.mark.parametrize("rule,name,k,loss", [c for c in lc.CASES if c[0] == "ftrl"], ids=lambda x: str(x))
def test_ftrl_epochs_are_well_conditioned_for_the_twin_alone(rule, name, k, loss):
    """The three shuffled epochs of the GPU test under the epochs' L1: the twin run in fp32 (ftrl_ref: what rounding alone does) ends
    within rel-L2 1e-6 of the fp64 twin in theta and zeta — a tenth of the GPU test's bound — and some of w and V is exactly zero."""
    from train_ref import rel
    case = lc.Case(rule, name, k, loss)
    a, orders = case.lay.a, lc.shuffled_orders(3, len(lc.batches(case.lay)), 3)
    s64 = case.epochs(case.start(), orders)
    s32 = case.epochs(fref.State(a["w0"], a["w"], a["v"], fref.INIT, fref.BETA, np.float32), orders)
    errs = [rel(getattr(s32, n), getattr(s64, n)) for n in ("v", "w", "zv", "zw")]
    assert max(errs) <= 1e-6, errs
    assert (s64.v == 0).any() and (s64.w == 0).any() and (s64.v != 0).any() and (s64.w != 0).any()


@pytest.mark.parametrize("rule,name,k,loss", [c for c in lc.CASES if lc.UPDATE_RULE[c[0]] == "adagrad"], ids=lambda x: str(x))
def test_adagrad_steps_move_as_check_step_expects(rule, name, k, loss):
    """test_gpu_adagrad.check_step's last assertion, of the twin: the largest change of V exceeds 1.5 eta sqrt(largest growth of n) — held here
    at 1.6, so that fp32 rounding cannot decide it on the device."""
    case = lc.Case(rule, name, k, loss)
    s0 = case.start()
    for r0, r1 in lc.batches(case.lay):
        s1 = case.step(s0.copy(), r0, r1)
        assert np.abs(s1.v - s0.v).max() > 1.6 * lc.ETA * np.sqrt((s1.nv - lc.INIT).max()), (r0, r1)


@pytest.mark.parametrize("loss", ["squared", "logistic"])
@pytest.mark.parametrize("k", [8, 32, 100])
def test_relational_hot_problem_and_its_ftrl_caps(k, loss):
    """relational_ref.base_problem(hot=True) as test_gpu_relational.py and test_gpu_ftrl.py use it: the option leaves every other
    array alone, both parts get a hot block by the library's rule, feature 99 sits in unreferenced user rows only, and the FTRL twin
    alone meets check_step's caps on every batch."""
    import relational_ref as rref
    p0, p = rref.base_problem(700 + k, k, loss), rref.base_problem(700 + k, k, loss, hot=True)
    assert all(np.array_equal(p0[n], p[n]) for n in ("y", "w", "v")) and np.array_equal(p0["blocks"][1]["col"], p["blocks"][1]["col"])
    assert np.array_equal(p0["maps"][0], p["maps"][0]) and np.array_equal(p0["maps"][1], p["maps"][1])
    want_u, want_p = rref.hot_layouts(p, 100)
    assert want_u["hot_pages"] >= 1 and set(rref.DEMO) <= set(want_u["hot_ids_all"]) and len(set(rref.DEMO) & set(want_u["hot_ids"])) >= 2
    assert want_p["hot_pages"] >= 1 and set(rref.PLAIN_HOT) <= set(want_p["hot_ids"]) and rref.DEMO_UNREFERENCED in want_u["hot_ids"]
    X = rref.dense(p["blocks"][0]["row_ptr"], p["blocks"][0]["col"], p["blocks"][0]["val"], p["n1"])
    share = (X[:, list(rref.DEMO)] != 0).mean(axis=0)
    assert (share >= 0.10).sum() >= 5 and (share <= 0.60).all()
    assert sorted(np.flatnonzero(X[:, rref.DEMO_UNREFERENCED])) == list(range(30, 37)) and p["maps"][0].max() < 30
    Xp = rref.dense(p["plain"]["row_ptr"], p["plain"]["col"], p["plain"]["val"], p["n1"])
    assert (((Xp[:, list(rref.PLAIN_HOT)] != 0).mean(axis=0) >= 0.15) & ((Xp[:, list(rref.PLAIN_HOT)] != 0).mean(axis=0) <= 0.55)).all()
    a = rref.flat(p)
    assert len(fref.cancelling_features(a["row_ptr"], a["col"], a["n1"])) == 0
    rule = fref.Rule(loss, False, fref.BETA, *fref.choose_l1(a, loss))
    s0 = fref.State(a["w0"], a["w"], a["v"], fref.INIT, fref.BETA)
    for b in range(4):
        s1 = fref.step(s0.copy(), a["row_ptr"], a["col"], a["val"], a["y"], b * 100, (b + 1) * 100, fref.ETA, *fref.L2, rule)
        near = fref.near_threshold(s0, s1, fref.ETA, rule)
        for name, g in (("w", s1.g[1]), ("v", s1.g[2])):
            touched = g != 0
            share = ((getattr(s1, name) == 0) & touched).sum() / max(touched.sum(), 1)
            assert 0.3 <= share <= 0.7, (name, b, share)
            assert near[name].sum() <= fref.ZERO_CAP * touched.sum(), (name, b, int(near[name].sum()), int(touched.sum()))


@pytest.mark.parametrize("rule", ["adagrad", "ftrl", "w_sgd"])
def test_random_shape_twins_alone(rule):
    """test_gpu_rules_by_layout.test_random_shapes_under_rules on the CPU: at its seed no twin diverges (the GPU test allows 2 of 24),
    the generator keeps its promises, and every FTRL case is well conditioned — the fp32 twin within rel-L2 1e-6 of the fp64 twin."""
    import test_gpu_rules_by_layout as t
    from train_ref import rel
    seen = []
    for case, a, batch_rows, br, hot, regs, eta, c in t.random_cases(rule, t.RANDOM_SEED, 24):
        assert 2 <= len(a["y"]) <= 600 and a["n1"] <= 3000 and batch_rows in (0, 7, 64, 300)
        if rule == "ftrl":
            assert np.diff(a["row_ptr"]).min() >= 2 and len(fref.cancelling_features(a["row_ptr"], a["col"], a["n1"])) == 0
        s = t.random_twin(a, rule, br, eta, regs, c)
        assert s is not None, case
        if rule == "ftrl":
            s32 = t.random_twin(a, rule, br, eta, regs, c, np.float32)
            assert max(rel(s32.v, s.v), rel(s32.w, s.w)) <= 1e-6, case
        seen.append((batch_rows, hot, regs[2] > 0, (c == 0).any() if c is not None else None))
    assert {b for b, _, _, _ in seen} == {0, 7, 64, 300} and sum(not h for _, h, _, _ in seen) in (4, 5)
    if rule == "adagrad":
        assert sum(d for _, _, d, _ in seen) == 18
    if rule == "w_sgd":
        assert all(z for _, _, _, z in seen)
