"""numpy restatement of fmhip_rank_metrics (include/fmhip_ranking.h) for tests/test_host_ranking.py and tests/test_gpu_ranking.py,
and the exact ranks of given rows in a block of scores (what fmhip_rank must count)."""
import numpy as np

FIELDS = ("hit_rate", "recall", "precision", "ndcg", "mrr", "map")


def rank_ref(ranks, k):
    """ranks: one integer array per context -> dict(k, contexts, skipped, relevant, hit_rate, recall, precision, ndcg, mrr, map)"""
    per = []
    for r in (np.sort(np.asarray(r, np.float64)) for r in ranks if len(r)):
        cut, n = r[r < k], len(r)
        idcg = (1.0 / np.log2(np.arange(min(n, k)) + 2.0)).sum()
        per.append((float(len(cut) > 0), len(cut) / n, len(cut) / k, (1.0 / np.log2(cut + 2.0)).sum() / idcg,
                    1.0 / (r[0] + 1.0), ((np.arange(n) + 1.0) / (r + 1.0)).sum() / n))
    out = dict(k=k, contexts=len(per), skipped=len(ranks) - len(per), relevant=sum(len(r) for r in ranks))
    out.update({f: (float(np.sum([p[i] for p in per])) / len(per) if per else 0.0) for i, f in enumerate(FIELDS)})
    return out


def ranks_of(S, targets, exclude=None):
    """S [M]: one context's scores; -> for every t in targets #{d not excluded, d != t: S[d] > S[t] or (S[d] == S[t] and d < t)},
    NaN below -inf and NaNs among themselves by row (the order of fmhip_topk)."""
    M = len(S)
    keep = np.ones(M, bool)
    if exclude is not None and len(exclude):
        keep[np.asarray(exclude, np.int64)] = False
    nan = np.isnan(S)
    key = np.where(nan, -np.inf, S)
    d = np.arange(M)
    out = []
    for t in targets:
        if nan[t]:
            above = ~nan | (d < t)
        else:
            above = ~nan & ((key > key[t]) | ((key == key[t]) & (d < t)))
        above[t] = False
        out.append(int((above & keep).sum()))
    return np.array(out, np.int32)
