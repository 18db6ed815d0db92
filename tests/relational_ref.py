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


def base_problem(seed, k, loss="squared", n_rows=400, plain=True, hot_refs=150):
    """The issue's base problem: a user block (J = 37, 0-6 nonzeros, ids [0, 100)), an item block (J = 90, 1-8 nonzeros, ids
    [100, 220)), a plain part (0-3 nonzeros, ids [220, 300)).  Item row 3 is referenced by `hot_refs` rows; user rows 30.. and item
    rows 80.. by nobody; item row 5 is empty (and referenced)."""
    rng = np.random.default_rng(seed)
    users = random_block(rng, 37, 0, 6, 0, 100)
    items = random_block(rng, 90, 1, 8, 100, 220, empty=(5,))
    mu = rng.integers(0, 30, n_rows)
    mi = rng.integers(0, 80, n_rows)
    mi[mi == 3] = 4
    mi[rng.choice(n_rows, size=min(hot_refs, n_rows), replace=False)] = 3
    mi[:2] = 5
    pl = random_block(rng, n_rows, 0, 3, 220, 300) if plain else None
    return make_problem(seed, n_rows, k, [users, items], [mu, mi], pl, 300, loss)


def build(fmhip, p, batch_rows=0):
    """-> (RelationalData, FMModel at the problem's parameters)."""
    rels = [fmhip.Relation((b["row_ptr"], b["col"], b["val"]), m) for b, m in zip(p["blocks"], p["maps"])]
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
