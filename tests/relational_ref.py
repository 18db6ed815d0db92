"""fp64 twin of the relational step (include/fmhip_relational.h), BY BLOCK CACHES — the formulas the device runs, not the flat
expansion — and the problems the relational tests share.

For parts b (relations, then the plain part under the identity mapping), data row r pointing at block row j_b(r):
    q_b[j] = sum_i v_i x_ji        yhat_b[j] = w0 + sum_i w_i x_ji + 1/2 sum_f (q_b[j]_f^2 - sum_i v_fi^2 x_ji^2)
    Q_r = sum_b q_b[j_b(r)]        yhat_r = w0 + sum_b (yhat_b[j_b(r)] - w0) + sum_{b < b'} <q_b[j_b(r)], q_b'[j_b'(r)]>
    P_b[j] = sum_{r: j_b(r) = j} e_r Q_r       e_b[j] = sum_{r: j_b(r) = j} e_r
    G_V[i] = sum_j x_ji P_b[j] - v_i sum_j x_ji^2 e_b[j]       G_w[i] = sum_j x_ji e_b[j]       G_0 = sum_r e_r
test_host_relational.py pins it to train_ref.step on expand() to 1e-12."""
import numpy as np

import train_ref as ref


def dense(rp, col, val, n1):
    """CSR rows -> dense [rows, n1] fp64 (a row stores a feature once in these problems)."""
    X = np.zeros((len(rp) - 1, n1))
    rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
    np.add.at(X, (rows, col), np.asarray(val, np.float64))
    return X


def parts_of(p):
    """The problem's parts as (dense X, mapping): the relations, then the plain part under the identity mapping."""
    out = [(dense(b["row_ptr"], b["col"], b["val"], p["n1"]), np.asarray(m, np.int64)) for b, m in zip(p["blocks"], p["maps"])]
    if p.get("plain") is not None:
        b = p["plain"]
        out.append((dense(b["row_ptr"], b["col"], b["val"], p["n1"]), np.arange(len(p["y"]), dtype=np.int64)))
    return out


def block_caches(s, X):
    """-> (q_b [J, k], yhat_b [J]) of one part at the state's parameters."""
    q = X @ s.v.T
    return q, s.w0 + X @ s.w + 0.5 * ((q * q).sum(1) - ((X * X) @ (s.v * s.v).T).sum(1))


def combine(s, parts, r0, r1):
    """-> (yhat [r1 - r0], Q [r1 - r0, k]) of the data rows [r0, r1) from the parts' caches."""
    Q = np.zeros((r1 - r0, s.v.shape[0]))
    yh = np.full(r1 - r0, s.w0)
    for X, mp in parts:
        q, yb = block_caches(s, X)
        j = mp[r0:r1]
        yh += (yb[j] - s.w0) + (q[j] * Q).sum(1)
        Q += q[j]
    return yh, Q


def predict(s, p):
    return combine(s, parts_of(p), 0, len(p["y"]))[0]


def residuals(s, p, r0, r1, loss):
    yh, _ = combine(s, parts_of(p), r0, r1)
    return ref.residuals(yh, p["y"][r0:r1], loss)


def gradient(s, p, r0, r1, loss):
    """-> (G_0, G_w [n1], G_V [k, n1], e) of the rows [r0, r1), assembled per part from (P_b, e_b)."""
    parts = parts_of(p)
    yh, Q = combine(s, parts, r0, r1)
    e = ref.residuals(yh, p["y"][r0:r1], loss)
    gw, gv = np.zeros_like(s.w), np.zeros_like(s.v)
    for X, mp in parts:
        Pb, eb = np.zeros((X.shape[0], Q.shape[1])), np.zeros(X.shape[0])
        np.add.at(Pb, mp[r0:r1], e[:, None] * Q)
        np.add.at(eb, mp[r0:r1], e)
        gv += (X.T @ Pb).T - s.v * ((X * X).T @ eb)[None, :]
        gw += X.T @ eb
    return e.sum(), gw, gv, e


def step(s, p, r0, r1, eta, reg0, regw, regv, rule=ref.Rule()):
    """One relational step of the rows [r0, r1) under `rule` (single rows), in place; -> s."""
    assert not rule.pairs
    g0, gw, gv, _ = gradient(s, p, r0, r1, rule.loss)
    b = float(r1 - r0)
    h0, hw, hv = g0 / b + reg0 * s.w0, gw / b + regw * s.w, gv / b + regv * s.v
    if rule.eps is None:
        s.w0, s.w, s.v = s.w0 - eta * h0, s.w - eta * hw, s.v - eta * hv
        return s
    t0, s.n0 = ref.adagrad_rule(np.float64(s.w0), np.float64(s.n0), h0, eta, rule.eps)
    s.w0 = float(t0)
    s.w, s.nw = ref.adagrad_rule(s.w, s.nw, hw, eta, rule.eps)
    s.v, s.nv = ref.adagrad_rule(s.v, s.nv, hv, eta, rule.eps)
    return s


def epochs(s, p, batch_rows, orders, eta, reg0, regw, regv, rule=ref.Rule()):
    n = len(p["y"])
    nb = (n + batch_rows - 1) // batch_rows
    for order in orders:
        for b in (range(nb) if order is None else order):
            step(s, p, b * batch_rows, min(n, (b + 1) * batch_rows), eta, reg0, regw, regv, rule)
    return s


# ---- problems -------------------------------------------------------------------------------------------------------

def random_block(rng, rows, lo, hi, id_lo, id_hi, empty=()):
    """`rows` CSR rows of lo..hi distinct features drawn from [id_lo, id_hi); the rows in `empty` store nothing."""
    rp, col, val = [0], [], []
    for j in range(rows):
        n = 0 if j in empty else int(rng.integers(lo, hi + 1))
        col.append(rng.choice(np.arange(id_lo, id_hi), size=n, replace=False).astype(np.int32))
        val.append(np.where(rng.random(n) < 0.5, 1.0, rng.uniform(0.1, 1.0, n)))
        rp.append(rp[-1] + n)
    return dict(row_ptr=np.asarray(rp, np.int64), col=np.concatenate(col).astype(np.int32), val=np.concatenate(val))


def make_problem(seed, n_rows, k, blocks, maps, plain, n1, loss="squared", scale=0.1):
    rng = np.random.default_rng(seed + 1000)
    y = rng.normal(0, 1.0, n_rows) if loss == "squared" else (rng.random(n_rows) < 0.4).astype(np.float64)
    return dict(k=k, n1=n1, w0=float(rng.normal(0, scale)), w=rng.normal(0, scale, n1), v=rng.normal(0, scale, (k, n1)), y=y, blocks=blocks,
                maps=[np.asarray(m, np.int32) for m in maps], plain=plain)


def base_problem(seed, k, loss="squared", n_rows=400, plain=True, hot_refs=150, hot=False):
    """The issue's base problem: a user block (J = 37, 0-6 nonzeros, ids [0, 100)), an item block (J = 90, 1-8 nonzeros, ids
    [100, 220)), a plain part (0-3 nonzeros, ids [220, 300)).  Item row 3 is referenced by `hot_refs` rows; user rows 30.. and item
    rows 80.. by nobody; item row 5 is empty (and referenced).
    hot (default off: every other case keeps its data): dense features on top, from a generator of their own — six "demographic"
    features (ids 94..99) in the user block, five of them in 15-60 % of its rows and id 99 in the seven rows nobody references and
    in no other (19 % of the block: its gradient is exactly zero); three features (ids 297..299) in 20-50 % of the plain part's rows.
    Built with hot_block=4 (the user block) and in several batches (the plain part) both hold a dense hot block: `hot_layouts`."""
    rng = np.random.default_rng(seed)
    users = random_block(rng, 37, 0, 6, 0, 100)
    items = random_block(rng, 90, 1, 8, 100, 220, empty=(5,))
    mu = rng.integers(0, 30, n_rows)
    mi = rng.integers(0, 80, n_rows)
    mi[mi == 3] = 4
    mi[rng.choice(n_rows, size=min(hot_refs, n_rows), replace=False)] = 3
    mi[:2] = 5
    pl = random_block(rng, n_rows, 0, 3, 220, 300) if plain else None
    if hot:
        hrng = np.random.default_rng(seed + 7000)
        users = with_dense_features(hrng, users, [94, 95, 96, 97, 98], hrng.uniform(0.15, 0.60, 5))
        users = with_dense_features(hrng, users, [DEMO_UNREFERENCED], [1.0], rows=range(30, 37), only=True)
        if plain:
            pl = with_dense_features(hrng, pl, list(PLAIN_HOT), hrng.uniform(0.20, 0.50, 3))
    return make_problem(seed, n_rows, k, [users, items], [mu, mi], pl, 300, loss)


DEMO = (94, 95, 96, 97, 98, 99)         # base_problem(hot=True): the user block's dense features ...
DEMO_UNREFERENCED = 99                  # ... the one that only rows nobody references hold
PLAIN_HOT = (297, 298, 299)             # ... and the plain part's


def with_dense_features(rng, block, ids, shares, rows=None, only=False):
    """The block with feature ids[i] added to a share shares[i] of `rows` (default: all) where the row does not hold it yet;
    only: and removed from every other row."""
    n = len(block["row_ptr"]) - 1
    rows = set(range(n) if rows is None else rows)
    rp, col, val = [0], [], []
    for j in range(n):
        c, x = block["col"][block["row_ptr"][j]:block["row_ptr"][j + 1]].tolist(), block["val"][block["row_ptr"][j]:block["row_ptr"][j + 1]].tolist()
        for f, share in zip(ids, shares):
            draw = rng.random() < share
            if j in rows and draw and f not in c:
                c.append(int(f))
                x.append(float(rng.uniform(0.1, 1.0)))
            if only and j not in rows and f in c:
                x.pop(c.index(f))
                c.remove(f)
        col += c
        val += x
        rp.append(len(col))
    return dict(row_ptr=np.asarray(rp, np.int64), col=np.asarray(col, np.int32), val=np.asarray(val, np.float64))


def hot_layouts(p, batch_rows, hot_block=4):
    """What ds.layout() must report for the user block (built single-batch with hot_block by name) and for the plain part (in batches
    of batch_rows) of base_problem(hot=True), by the library's rule as layout_cases.expected_layout restates it."""
    import layout_cases as lc
    return (lc.expected_layout(dict(p["blocks"][0], n1=p["n1"]), dict(batch_rows=0, hot_block=hot_block)),
            lc.expected_layout(dict(p["plain"], n1=p["n1"]), dict(batch_rows=batch_rows)))


def build(fmhip, p, batch_rows=0, hot_block=None):
    """-> (RelationalData, FMModel at the problem's parameters).  hot_block: relation 0's block is a DataSet built with a dense hot
    block asked for by name (a single-batch dataset gets none by default)."""
    rels = [fmhip.Relation((b["row_ptr"], b["col"], b["val"]), m) for b, m in zip(p["blocks"], p["maps"])]
    if hot_block:
        b = p["blocks"][0]
        rels[0] = fmhip.Relation(fmhip.DataSet(b["row_ptr"], b["col"], b["val"], np.zeros(len(b["row_ptr"]) - 1), batch_rows=0, hot_block=hot_block),
                                 p["maps"][0])
    pl = None if p.get("plain") is None else fmhip.Features(p["plain"]["row_ptr"], p["plain"]["col"], p["plain"]["val"])
    rd = fmhip.RelationalData(p["y"], rels, plain=pl, batch_rows=batch_rows)
    fm = fmhip.FMModel(p["n1"] - 1, p["k"])
    fm.w0, fm.w, fm.v = p["w0"], p["w"], p["v"]
    return rd, fm


def flat(p):
    """The expansion as arrays (numpy only: what RelationalData.expand() must return)."""
    n = len(p["y"])
    srcs = [(b, np.asarray(m, np.int64)) for b, m in zip(p["blocks"], p["maps"])]
    if p.get("plain") is not None:
        srcs.append((p["plain"], np.arange(n)))
    rp, col, val = [0], [], []
    for r in range(n):
        for b, m in srcs:
            a, z = b["row_ptr"][m[r]], b["row_ptr"][m[r] + 1]
            col.extend(b["col"][a:z].tolist())
            val.extend(b["val"][a:z].tolist())
        rp.append(len(col))
    return dict(row_ptr=np.asarray(rp, np.int64), col=np.asarray(col, np.int32), val=np.asarray(val, np.float64), y=p["y"], k=p["k"], n1=p["n1"],
                w0=p["w0"], w=p["w"], v=p["v"])
