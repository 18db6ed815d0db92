"""A numpy twin of the AUC kernels (include/fmhip_metrics.h, sparkfm_amd/csrc/fm_auc.h): the 64-bit word of a row, a sort, and
the run / group formulas in Python ints — and, beside it, the O(n^2) pair count the twin is itself checked against."""
import math

import numpy as np

FIELDS = ("u2", "pairs", "positives", "negatives", "groups", "groups_scored")


def score_keys(scores):
    """float32 scores -> the order-preserving uint32 keys: NaN -> 0, then -Inf < ... < -0 = +0 < ... < +Inf."""
    s = np.ascontiguousarray(scores, np.float32).reshape(-1) + np.float32(0.0)       # -0 -> +0
    u = s.view(np.uint32)
    key = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
    return np.where(np.isnan(s), np.uint32(0), key).astype(np.uint32)


def words(scores, labels, groups=None):
    """group << 33 | key << 1 | [label > 0], one uint64 per row."""
    key = score_keys(scores).astype(np.uint64)
    t = (np.ascontiguousarray(labels, np.float32).reshape(-1) > 0).astype(np.uint64)
    g = np.zeros(len(key), np.uint64) if groups is None else np.asarray(groups).astype(np.uint64)
    return (g << np.uint64(33)) | (key << np.uint64(1)) | t


def auc_ref(scores, labels, groups=None):
    """-> the fields of fmhip_auc_result as a dict (the integers exact; gauc summed group by group in ascending id order)."""
    W = np.sort(words(scores, labels, groups))
    n = len(W)
    out = dict(u2=0, pairs=0, positives=0, negatives=0, groups=0, groups_scored=0, auc=math.nan, gauc=math.nan)
    if n == 0:
        return out
    neg = (~W & np.uint64(1)).astype(np.int64)
    cneg = np.concatenate([[0], np.cumsum(neg)])                                    # negatives before position p, p = 0 .. n
    run_head = np.concatenate([[True], (W[1:] >> np.uint64(1)) != (W[:-1] >> np.uint64(1))])
    grp_head = np.concatenate([[True], (W[1:] >> np.uint64(33)) != (W[:-1] >> np.uint64(33))])
    rstart = np.flatnonzero(run_head)
    rend = np.concatenate([rstart[1:], [n]])
    A = []                                                                            # A_r = pos_r * (2 cneg(start) + neg_r)
    for s, e in zip(rstart.tolist(), rend.tolist()):
        nb = int(cneg[s])
        ng = int(cneg[e]) - nb
        A.append(((e - s) - ng) * (2 * nb + ng))
    SA = [0]
    for a in A:
        SA.append(SA[-1] + a)
    gstart = np.flatnonzero(grp_head)
    gend = np.concatenate([gstart[1:], [n]])
    run_of = np.cumsum(run_head) - 1                                                  # the run a position belongs to
    num, rows_scored = 0.0, 0
    for s, e in zip(gstart.tolist(), gend.tolist()):
        r0, r1 = int(run_of[s]), int(run_of[e - 1]) + 1
        nb = int(cneg[s])
        ng = int(cneg[e]) - nb
        ps = (e - s) - ng
        if ps > 0 and ng > 0:
            u2 = SA[r1] - SA[r0] - 2 * nb * ps
            out["u2"] += u2
            out["pairs"] += ps * ng
            out["groups_scored"] += 1
            rows_scored += e - s
            num += float(e - s) * (float(u2) / (2.0 * float(ps * ng)))
    out["groups"] = len(gstart)
    out["negatives"] = int(cneg[n])
    out["positives"] = n - out["negatives"]
    if out["pairs"]:
        out["auc"] = float(out["u2"]) / (2.0 * float(out["pairs"]))
    if out["groups_scored"] == 1:
        out["gauc"] = out["auc"]                                                      # the weighted mean of one number
    elif out["groups_scored"] > 1:
        out["gauc"] = num / float(rows_scored)
    return out


def _order(a, b):
    """-1 / 0 / +1 as float32 a ranks below / ties with / ranks above b: NaN below everything and equal to NaN, -0 == +0."""
    an, bn = math.isnan(a), math.isnan(b)
    if an or bn:
        return 0 if an and bn else (-1 if an else 1)
    return (a > b) - (a < b)


def auc_brute(scores, labels, groups=None):
    """The same fields by counting every (positive, negative) pair of a group: O(n^2), for small n."""
    s = [float(x) for x in np.asarray(scores, np.float32).reshape(-1)]
    t = [float(x) > 0 for x in np.asarray(labels, np.float32).reshape(-1)]
    g = [0] * len(s) if groups is None else [int(x) for x in groups]
    out = dict(u2=0, pairs=0, positives=sum(t), negatives=len(t) - sum(t), groups=len(set(g)), groups_scored=0, auc=math.nan,
               gauc=math.nan)
    num, rows_scored, last = 0.0, 0, math.nan
    for gid in sorted(set(g)):
        rows = [i for i in range(len(s)) if g[i] == gid]
        pos, neg = [i for i in rows if t[i]], [i for i in rows if not t[i]]
        if not pos or not neg:
            continue
        u2 = sum(1 + _order(s[p], s[q]) for p in pos for q in neg)
        out["u2"] += u2
        out["pairs"] += len(pos) * len(neg)
        out["groups_scored"] += 1
        rows_scored += len(rows)
        last = float(u2) / (2.0 * float(len(pos) * len(neg)))
        num += float(len(rows)) * last
    if out["pairs"]:
        out["auc"] = float(out["u2"]) / (2.0 * float(out["pairs"]))
    if out["groups_scored"] == 1:
        out["gauc"] = last
    elif out["groups_scored"] > 1:
        out["gauc"] = num / float(rows_scored)
    return out


def same(a, b):
    """two floats equal bit for bit, NaN equal to NaN"""
    return (math.isnan(a) and math.isnan(b)) or a == b
