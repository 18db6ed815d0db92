"""Named dataset layouts that reach the layout-specific code paths (the dense hot block's page 0 and gradient-side pages, a hot
row with a zero gradient, the rows-only update with hot ids, row-blocked transposes, a named single-batch hot block), shared by
test_host_layout_cases.py (which recomputes every claim in numpy) and test_gpu_rules_by_layout.py (which asserts ds.layout()).

Pure numpy.  `layout(name, k, loss)` -> Layout: the problem dict train_ref.make takes, how to build the dataset, and what
ds.layout() must report.  The rows of a layout do not depend on k or on the loss; its parameters and labels do.

The library's rule (fmhip_host.cpp, choose_hot_block), which `expected_layout` restates: a feature is a candidate at >= 2.5 % of
the rows, candidates rank by descending count (ties: ascending id); page 0 (dense on both sides) takes the leading candidates
at >= 10 %, at most 16, and exists only with two or more of them; the gradient-side pages take the next 16 * (pages - 1); a
candidate that occurs twice in a row or with a stored zero is refused.  A single-batch dataset gets a hot block only when it is
asked for by name (hot_block >= 1), a row-blocked one gets page 0 only."""
from collections import namedtuple

import numpy as np

from test_gpu_parity import hot_problem

HOT_T = 16                      # slots per page (kHotT)
DEFAULT_PAGES = 4               # FMHIP_TUNE_HOT_PAGES as the library starts

# a: the problem; build: DataSet keywords (batch_rows, hot_block, row_block_rows); hot_ids / hot_ids_all: page 0's ids / every page's,
# ascending; hot_pages; absent: {batch: ids of hot features no row of that batch holds}; flat: the model runs the flat-address kernels
Layout = namedtuple("Layout", "name a build hot_ids hot_ids_all hot_pages absent flat")

NAMES = ("page0", "pages", "absent", "wide", "all_hot_wide", "named_single", "row_blocked", "flat_page0", "flat_wide")

# seeds chosen on the CPU (test_host_layout_cases.py holds every claim and every FTRL cap for them)
SEEDS = dict(page0=4101, pages=4202, wide=4303, all_hot_wide=5)


def _labels(a, seed, loss):
    if loss == "logistic":
        a["y"] = (np.random.default_rng(seed + 1).random(len(a["y"])) < 0.4).astype(np.float64)
    a["val"] = np.asarray(a["val"], np.float32).astype(np.float64)          # exactly representable in fp32
    return a


def _drop(a, feature, r0, r1):
    """The problem without `feature` in the rows [r0, r1)."""
    rp, col, val = a["row_ptr"], a["col"], a["val"]
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    keep = ~((col == feature) & (rows >= r0) & (rows < r1))
    new_rp = np.zeros_like(rp)
    np.cumsum(np.bincount(rows[keep], minlength=len(rp) - 1), out=new_rp[1:])
    return dict(a, row_ptr=new_rp, col=col[keep], val=val[keep])


def _all_hot_wide(k):
    """test_rows_only_update_when_every_feature_sits_in_the_hot_block's data: 40 rows that all hold the same 30 of 700 features."""
    rng = np.random.default_rng(SEEDS["all_hot_wide"])
    n_rows, n1, feats = 40, 700, rng.choice(700, size=30, replace=False).astype(np.int32)
    row_ptr = np.arange(n_rows + 1, dtype=np.int64) * 30
    col = np.concatenate([rng.permutation(feats) for _ in range(n_rows)]).astype(np.int32)
    val = rng.uniform(0.1, 1.0, len(col))
    return dict(k=k, n1=n1, w0=0.1, w=rng.normal(0, 0.1, n1), v=rng.normal(0, 0.1, (k, n1)), row_ptr=row_ptr, col=col, val=val,
                y=rng.normal(0, 1.0, n_rows)), np.sort(feats)


def expected_layout(a, build):
    """What ds.layout() must report for the problem under these build keywords, by the rule in the module's docstring:
    dict of hot_ids, hot_ids_all (ascending), hot_pages, nnz_sparse, nnz_sparse_backward."""
    rp, col, val = np.asarray(a["row_ptr"], np.int64), np.asarray(a["col"], np.int64), np.asarray(a["val"], np.float64)
    n_rows, nnz = len(rp) - 1, len(col)
    br = build.get("batch_rows", 0)
    nb = 1 if br <= 0 or br >= n_rows else (n_rows + br - 1) // br
    hb = build.get("hot_block")
    none = dict(hot_ids=[], hot_ids_all=[], hot_pages=0, nnz_sparse=nnz, nnz_sparse_backward=nnz)
    if hb is False or hb == 0 or (nb == 1 and hb is None) or nnz == 0:
        return none
    max_pages = DEFAULT_PAGES if hb is None or hb is True else int(hb)
    if build.get("row_block_rows"):
        max_pages = 1
    cnt = np.bincount(col, minlength=a["n1"])
    rows = np.repeat(np.arange(n_rows), np.diff(rp))
    key = rows * a["n1"] + col
    twice = np.unique(col[np.isin(key, key[np.flatnonzero(np.diff(np.sort(key)) == 0)])]) if nnz > 1 else np.zeros(0, np.int64)
    refused = set(twice.tolist()) | set(np.unique(col[val.astype(np.float32) == 0]).tolist())
    cand = [int(f) for f in np.flatnonzero(cnt * 40 >= n_rows)]
    cand.sort(key=lambda f: (-cnt[f], f))
    while True:
        p0 = 0
        while p0 < len(cand) and p0 < HOT_T and cnt[cand[p0]] * 10 >= n_rows:
            p0 += 1
        used = 0 if p0 < 2 else p0 + min(len(cand) - p0, HOT_T * (max_pages - 1))
        bad = [f for f in cand[:used] if f in refused]
        if not bad:
            break
        cand = [f for f in cand if f not in bad]
    if not used:
        return none
    ids0, ids_all = sorted(cand[:p0]), sorted(cand[:used])
    return dict(hot_ids=ids0, hot_ids_all=ids_all, hot_pages=1 + (used - p0 + HOT_T - 1) // HOT_T,
                nnz_sparse=int((~np.isin(col, ids0)).sum()), nnz_sparse_backward=int((~np.isin(col, ids_all)).sum()))


def batches(lay):
    """[(r0, r1)] of the layout's batches."""
    n, br = len(lay.a["y"]), lay.build.get("batch_rows", 0)
    br = n if br <= 0 or br > n else br
    return [(r0, min(n, r0 + br)) for r0 in range(0, n, br)]


def cold_columns(lay, b):
    """The distinct features of batch b that are not in the hot block: what the batch's transposes hold (n_cols)."""
    r0, r1 = batches(lay)[b]
    c = lay.a["col"][lay.a["row_ptr"][r0]:lay.a["row_ptr"][r1]]
    return np.setdiff1d(np.unique(c), lay.hot_ids_all)


def few_rows(lay, b):
    """step_apply's test for the rows-only update of batch b: 2 * (cold columns + 16 * pages) <= n1."""
    return 2 * (len(cold_columns(lay, b)) + HOT_T * lay.hot_pages) <= lay.a["n1"]


def layout(name, k, loss="squared", pairs=False):
    """The named layout at k factors (see the table in test_gpu_rules_by_layout.py).  pairs: batches of an even row count (298 in
    place of 297: still no multiple of 16; the last batch then has 8 rows) — a batch must not cut a pair."""
    flat = name.startswith("flat_")
    base = name[5:] if flat else name
    absent = {}
    if base in ("page0", "absent", "named_single", "row_blocked"):
        # 1200 x 500, 12 features in 15-95 % of the rows: page 0 with 4 unused slots; batches of 297 rows (5 of them, the last of 12
        # rows; pairs: 298 and 8): no multiple of 64 or 16, so the block product's last workgroup and last wave are partial
        seed = SEEDS["page0"]
        a, hot = hot_problem(seed, 1200, 500, k, 12)
        br = 298 if pairs else 297
        build = dict(batch_rows=br)
        if base == "absent":
            # the two most frequent hot features leave every row of batch 1, the third leaves the last batch: all stay >= 10 % overall
            cnt = np.bincount(a["col"], minlength=a["n1"])
            top = [int(f) for f in sorted(hot, key=lambda f: (-cnt[f], f))[:3]]
            a = _drop(_drop(a, top[0], br, 2 * br), top[1], br, 2 * br)
            a = _drop(a, top[2], 4 * br, 1200)
            absent = {1: sorted(top[:2]), 4: [top[2]]}
        if base == "named_single":
            build = dict(batch_rows=0, hot_block=4)
        if base == "row_blocked":
            build = dict(batch_rows=br, row_block_rows=128)
        ids0, ids_all, pages = sorted(int(x) for x in hot), sorted(int(x) for x in hot), 1
    elif base == "pages":
        # 1500 x 600, 40 hot features, 25 of them in 6.5-9 % of the rows: a partly filled page 0 (15 ids), two gradient-side pages
        seed = SEEDS["pages"]
        a, hot = hot_problem(seed, 1500, 600, k, 40, n_low=25)
        build = dict(batch_rows=400, hot_block=8)
        ids0, ids_all, pages = sorted(int(x) for x in hot[:15]), sorted(int(x) for x in hot), 3
    elif base == "wide":
        # 1200 x 6000, 8 hot features, batches of 300: a batch touches a few hundred of 6000 rows — the rows-only update, n_hot = 16
        seed = SEEDS["wide"]
        a, hot = hot_problem(seed, 1200, 6000, k, 8)
        build = dict(batch_rows=300)
        ids0, ids_all, pages = sorted(int(x) for x in hot), sorted(int(x) for x in hot), 1
    else:
        assert base == "all_hot_wide", name
        seed = SEEDS["all_hot_wide"]
        a, hot = _all_hot_wide(k)
        build = dict(batch_rows=10)
        cnt_order = sorted(int(x) for x in hot)            # every count is 40: the ranking is by id
        ids0, ids_all, pages = cnt_order[:16], cnt_order, 2
    return Layout(name, _labels(a, seed, loss), build, ids0, ids_all, pages, absent, flat)


def build_without_hot_block(lay):
    """The control of a case: the same data with the hot block off."""
    return dict(lay.build, hot_block=False)


# ---- the covering table of test_gpu_rules_by_layout.py: (rule, layout, k, loss) ------------------------------------------------

RULES = ("adagrad_decay", "adagrad", "ftrl", "w_sgd", "w_adagrad", "w_pairs")
UPDATE_RULE = dict(adagrad_decay="adagrad", adagrad="adagrad", w_adagrad="adagrad", ftrl="ftrl", w_sgd="sgd", w_pairs="sgd")
MAIN = ("page0", "pages", "absent", "wide")          # every k meets these under every update rule
KS = (8, 32, 64, 100)                                # Kp 32 with w packed; k = Kp; four pages per pass; Kp 128
LOSSES = ("squared", "logistic")


def _cases():
    out = []
    for li, lay in enumerate(MAIN):
        k_at = lambda j: KS[(li + j) % 4]            # noqa: E731
        picks = [("ftrl", k) for k in KS]
        picks += [("w_sgd", k_at(0)), ("w_pairs", k_at(1)), ("w_sgd", k_at(2)), ("w_pairs", k_at(3))]
        picks += [("adagrad_decay", k_at(0)), ("adagrad", k_at(1)), ("w_adagrad", k_at(2)),
                  (("adagrad", "adagrad_decay", "w_adagrad", "adagrad")[li], k_at(3))]
        out += [(rule, lay, k, LOSSES[(li + j) % 2]) for j, (rule, k) in enumerate(picks)]
    for oi, lay in enumerate(n for n in NAMES if n not in MAIN):
        out += [(rule, lay, KS[(oi + ri) % 4], LOSSES[(oi + ri) % 2]) for ri, rule in enumerate(RULES)]
    out.append(("adagrad", "pages", 256, "squared"))     # Kp 256: one page per pass
    return out


CASES = _cases()


def table():
    """The covering table as text: one line per layout, `rule k loss-initial` entries."""
    lines = []
    for lay in NAMES:
        cells = ["%s %d%s" % (r, k, loss[0]) for r, n, k, loss in CASES if n == lay]
        lines.append("    %-13s %s" % (lay, ", ".join(cells)))
    return "\n".join(lines)


# ---- the rules' settings and twins, shared by the CPU check of the caps and the GPU tests -----------------------------------------

ETA, INIT, EPS = 0.05, 0.1, 1e-10
EPOCH_L1 = (0.1, 0.01)
REGS = (1e-3, 2e-3, 3e-3)
ROWS_ONLY_LAYOUTS = ("wide", "all_hot_wide", "flat_wide")


class Case:
    """One line of the table with everything its twin needs: the layout, the example weights c (weighted rules), the regularisers,
    the twin's rule, and for FTRL the L1 pair ftrl_ref.choose_l1 gives for the whole dataset taken as one batch."""

    def __init__(self, rule, name, k, loss):
        import ftrl_ref as fref
        import train_ref as ref
        import weight_ref as wref
        self.rule, self.name, self.k, self.loss = rule, name, k, loss
        self.pairs = rule == "w_pairs"
        self.lay = layout(name, k, loss, pairs=self.pairs)
        a, n = self.lay.a, len(self.lay.a["y"])
        self.c = None
        if rule.startswith("w_"):
            # (all_hot_wide: ten-row batches of rows that hold every feature, weights up to 3.5 — g^2 is large against the accumulators'
            # start, and test_gpu_adagrad.check_step's "it moved by AdaGrad's steps" holds for the twin at few weight seeds: 926 is one)
            seed = 926 if name == "all_hot_wide" else 900 + k + len(name)
            self.c = np.repeat(wref.draw_weights(seed, n // 2), 2) if self.pairs else wref.draw_weights(seed, n)
        # AdaGrad without decay, and weighted AdaGrad on the wide layouts: the rows-only update where step_apply allows it
        no_decay = rule == "adagrad" or (rule == "w_adagrad" and name in ROWS_ONLY_LAYOUTS)
        self.regs = (0.0, 0.0, 0.0) if no_decay else REGS
        self.update = UPDATE_RULE[rule]
        if rule == "ftrl":
            self.regs = fref.L2
            self.l1 = fref.choose_l1(a, loss)
            self.twin_rule = fref.Rule(loss, False, fref.BETA, *self.l1)
            # the epochs' L1: test_gpu_ftrl.test_epochs_vs_twin's (0.1, 0.01), not the one-step median.  Once the L1 has zeroed factor
            # f of every OTHER feature of a row, the row's gradient of v_fi is e x (q_f - v_fi x) = 0 in exact arithmetic and rounding
            # noise or zero in floating point — ftrl_ref.one_step_problem's discontinuity, reached through training.  At the median L1
            # (and still at choose_l1's share 0.1 on the wide layout) three epochs get there, and the fp32 twin ALONE ends up to 1e-2
            # (rel-L2 of v) from the fp64 twin; test_host_layout_cases.py holds the fp32 twin to 1e-6 at this L1, for every case
            self.l1_epochs = EPOCH_L1
            self.twin_rule_epochs = fref.Rule(loss, False, fref.BETA, *self.l1_epochs)
        else:
            self.twin_rule = ref.Rule(loss, self.pairs, EPS if self.update == "adagrad" else None)

    def start(self):
        import ftrl_ref as fref
        import train_ref as ref
        a = self.lay.a
        if self.rule == "ftrl":
            return fref.State(a["w0"], a["w"], a["v"], fref.INIT, fref.BETA)
        return ref.State(a["w0"], a["w"], a["v"], INIT if self.update == "adagrad" else 0.0)

    def step(self, s, r0, r1, rule=None):
        """One twin step of the rows [r0, r1), in place; -> s.  rule: in place of the case's one-step rule (the epochs' L1)."""
        import ftrl_ref as fref
        import train_ref as ref
        import weight_ref as wref
        a = self.lay.a
        if self.rule == "ftrl":
            return fref.step(s, a["row_ptr"], a["col"], a["val"], a["y"], r0, r1, ETA, *self.regs, rule or self.twin_rule)
        if self.c is not None:
            return wref.step(s, a["row_ptr"], a["col"], a["val"], a["y"], self.c, r0, r1, ETA, *self.regs, self.twin_rule)
        return ref.step(s, a["row_ptr"], a["col"], a["val"], a["y"], r0, r1, ETA, *self.regs, self.twin_rule)

    def epochs(self, s, orders):
        """Epochs of the layout's batches in orders[e] (None: ascending), FTRL under the epochs' L1; -> s."""
        bs = batches(self.lay)
        for order in orders:
            for b in (range(len(bs)) if order is None else order):
                self.step(s, *bs[b], rule=getattr(self, "twin_rule_epochs", None))
        return s


def shuffled_orders(shuffle_seed, n_batches, epochs):
    """HipSGD.batch_order's orders of the first `epochs` epochs."""
    return [np.random.Generator(np.random.PCG64([shuffle_seed, e])).permutation(n_batches).tolist() for e in range(epochs)]
