"""Ranking metrics of predictions that are already on the host (include/fmhip_metrics.h) — what a data-parallel caller uses
after gathering its ranks' predictions; a model over a dataset goes through ``FMModel.computeAUC`` instead."""
import ctypes as C

import numpy as np

from . import _ffi


def auc(scores, labels, groups=None, device=0):
    """ROC AUC and per-group AUC of `scores` against the labels t = [labels > 0], ranked on the GPU, exactly (fmhip_auc_scores):
    a dict of u2, pairs, positives, negatives, groups, groups_scored, auc, gauc.  Scores are compared as float32: -0 ties with
    +0, NaN ranks below -inf and ties with NaN.  `groups`: None (one group), or one integer id in [0, 2^31) per row."""
    s = np.ascontiguousarray(scores, np.float32).reshape(-1)
    y = np.ascontiguousarray(labels, np.float32).reshape(-1)
    if s.shape != y.shape:
        raise ValueError("scores and labels differ in length: %d, %d" % (len(s), len(y)))
    g = _ffi.group_ids(groups, len(s))
    res = _ffi.AucResult()
    _ffi.check(_ffi.load().fmhip_auc_scores(int(device), len(s), _ffi.ptr(s), _ffi.ptr(y), _ffi.ptr(g), C.byref(res)))
    return res.as_dict()
