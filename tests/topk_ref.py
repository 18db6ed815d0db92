"""fp64 reference of the top-K recommendation calls (fmhip_topk / fmhip_pair_scores) for tests/test_host_topk.py and
tests/test_gpu_topk.py: row sets over disjoint id ranges, the pair identity's right-hand side from the oracle's predict,
the project's score tolerance, and the "valid top-K up to rounding" check."""
import numpy as np

import oracle

TOL_Y = 1e-5      # as tests/test_gpu_parity.py: |d| <= TOL_Y * (1 + sum |terms|)


def field_rows(seed, n_rows, fields, empty=(), keep=0.8, half=True):
    """Rows holding at most one id from each field (lo, hi) — ids hi exclusive — so ids are distinct within a row; every
    entry is kept with probability `keep`; rows in `empty` hold nothing.  Values 1, or 1/2 .. 1 (half=False: uniform).
    -> dict(row_ptr, col, val)"""
    rng = np.random.default_rng(seed)
    F = len(fields)
    cols = np.stack([rng.integers(lo, hi, n_rows) for lo, hi in fields], axis=1).astype(np.int32)
    vals = np.where(rng.random((n_rows, F)) < 0.5, 1.0, 0.5 if half else rng.uniform(0.1, 1.0, (n_rows, F)))
    mask = rng.random((n_rows, F)) < keep
    mask[:, 0] |= ~mask.any(axis=1)             # no accidental empty rows: only the named ones
    if len(empty):
        mask[np.asarray(empty, np.int64)] = False
    row_ptr = np.zeros(n_rows + 1, np.int64)
    np.cumsum(mask.sum(axis=1), out=row_ptr[1:])
    return dict(row_ptr=row_ptr, col=np.ascontiguousarray(cols[mask]), val=np.ascontiguousarray(vals[mask]).astype(np.float64))


def params(seed, n1, k, scale=0.1):
    rng = np.random.default_rng(seed)
    return float(rng.normal(0, scale)), rng.normal(0, scale, n1), rng.normal(0, scale, (k, n1))


def row_stats(w0, w, v, r):
    """-> (predict [rows] from the oracle, q [rows, k], sum of |terms| [rows] as tests/test_gpu_parity.py: term_scale forms it)"""
    n = len(r["row_ptr"]) - 1
    k = v.shape[0]
    yhat = oracle.predict(w0, w, v, r["row_ptr"], r["col"], r["val"]) if n else np.zeros(0)
    vx = (v[:, r["col"]] * r["val"]).T                        # [nnz, k]
    lens = np.diff(r["row_ptr"])
    ne = lens > 0
    starts = r["row_ptr"][:-1][ne]

    def rowsum(x):                                            # per-row sums of consecutive entries (empty rows: 0)
        out = np.zeros((n,) + x.shape[1:])
        if len(starts):
            out[ne] = np.add.reduceat(x, starts, axis=0)
        return out
    q, a1, a2 = rowsum(vx), rowsum(np.abs(vx)), rowsum(vx * vx)
    lin = rowsum(np.abs(w[r["col"]] * r["val"]))
    terms = abs(w0) + lin + 0.5 * ((a1 ** 2).sum(axis=1) + a2.sum(axis=1))
    return yhat, q, terms


def pair_ref(w0, w, v, ctx, cand, rows=None):
    """The identity's right-hand side and its tolerance: S [B, M], tol [B, M] (rows: only these contexts)."""
    yc, qc, tc = row_stats(w0, w, v, ctx)
    yd, qd, td = row_stats(w0, w, v, cand)
    if rows is not None:
        yc, qc, tc = yc[rows], qc[rows], tc[rows]
    S = yc[:, None] + yd[None, :] - w0 + qc @ qd.T
    tol = TOL_Y * (1.0 + tc[:, None] + td[None, :] + abs(w0) + np.abs(qc) @ np.abs(qd).T)
    return S, tol


def joined(ctx, cand, pairs):
    """The explicit rows "c's entries, then d's" for the (c, d) in pairs -> dict(row_ptr, col, val)."""
    col, val, ptr = [], [], [0]
    for c, d in pairs:
        for r, i in ((ctx, c), (cand, d)):
            s = slice(r["row_ptr"][i], r["row_ptr"][i + 1])
            col.append(r["col"][s])
            val.append(r["val"][s])
        ptr.append(ptr[-1] + len(col[-2]) + len(col[-1]))
    return dict(row_ptr=np.asarray(ptr, np.int64), col=np.concatenate(col).astype(np.int32) if col else np.zeros(0, np.int32),
                val=np.concatenate(val) if val else np.zeros(0))


def check_topk(idx, score, S, tol, k, exclude=None, contexts=None):
    """`idx`, `score` [B, k] are a valid top-K of S [B, M] up to rounding (tol [B, M]), for every context (contexts: the rows
    of idx / score that S's rows stand for).  No exemption for near-ties: every statement holds with the stated slack."""
    M = S.shape[1]
    rows = range(S.shape[0]) if contexts is None else contexts
    for si, c in enumerate(rows):
        ex = np.unique(np.asarray(exclude[c], np.int64)) if exclude is not None else np.zeros(0, np.int64)
        ids, sc = idx[c], score[c]
        n = min(k, M - len(ex))
        assert (ids[n:] == -1).all() and np.isneginf(sc[n:]).all(), (c, ids, sc)
        ids, sc = ids[:n].astype(np.int64), sc[:n]
        assert ((ids >= 0) & (ids < M)).all() and len(np.unique(ids)) == n, (c, ids)
        assert not np.isin(ids, ex).any(), (c, ids)
        assert (np.abs(sc - S[si, ids]) <= tol[si, ids]).all(), (c, float((np.abs(sc - S[si, ids]) / tol[si, ids]).max()))
        assert (np.diff(sc) <= 0).all(), (c, sc)
        tie = np.diff(sc) == 0
        assert (np.diff(ids)[tie] > 0).all(), (c, ids, sc)
        rest = np.ones(M, bool)
        rest[ids] = False
        rest[ex] = False
        if n < k:
            assert not rest.any(), c
            continue
        jmin = int(np.argmin(S[si, ids]))
        bound = S[si, ids[jmin]] + tol[si, rest] + tol[si, ids[jmin]]
        assert (S[si, rest] <= bound).all(), (c, float((S[si, rest] - bound).max()))
