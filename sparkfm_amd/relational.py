"""Relation / RelationalData — relational data for block-structure FM (include/fmhip_relational.h).

The reference left S/fm/bs/* a stub (``Relation.cache = null``) and its relational learner commented out; what the stub was
heading for is Rendle's block-structure FM.  A ``Relation`` is a block of feature rows (the users with all their features, the
items with theirs) and a mapping from data rows to block rows; a ``RelationalData`` is N labels, one or more relations and an
optional plain part (features of the data rows themselves).  It stands for the flat ``DataSet`` whose row r holds relation 0's
entries of block row ``mapping_0[r]``, then relation 1's, ..., then the plain part's (``expand()``) — without ever building it:
training walks every block once per step, and scoring runs each block's forward once.
"""
import ctypes as C

import numpy as np

from . import _ffi
from .dataset import DataSet, Features


def _as_features(features):
    """Features | (row_ptr, col, val) | rows of (indices, values) -> Features."""
    if isinstance(features, Features):
        return features
    if (isinstance(features, tuple) and len(features) == 3 and not isinstance(features[0], tuple)
            and (len(features[0]) == 0 or np.ndim(features[0][0]) == 0)):       # row_ptr's entries are scalars, a row's first item is its indices
        return Features(*features)
    ptr, cols, vals = [0], [], []
    for idx, v in features:
        idx, v = np.asarray(idx, np.int32), np.asarray(v, np.float64)
        if len(idx) != len(v):
            raise ValueError("index/value length mismatch in a block row")
        cols.append(idx)
        vals.append(v)
        ptr.append(ptr[-1] + len(idx))
    return Features(np.asarray(ptr, np.int64), np.concatenate(cols) if cols else np.zeros(0, np.int32),
                    np.concatenate(vals) if vals else np.zeros(0, np.float64))


class Relation:
    """A block of J feature rows and a mapping: data row r uses block row ``mapping[r]``.  ``features``: a ``Features`` (a
    ``DataSet`` is taken as the block itself — it must be a single-batch training dataset), (row_ptr, col, val), or an iterable
    of (indices, values) rows.  One Relation may serve several RelationalData (training and held-out rows over the same users)
    when its mapping is replaced: ``relation.remap(mapping)`` shares the block."""

    def __init__(self, features, mapping, name="relation", device=0):
        if isinstance(features, DataSet):
            self.block = features
        else:
            f = _as_features(features)
            self.block = DataSet(f.row_ptr, f.col, f.val, np.zeros(f.size, f.val.dtype), name=name, batch_rows=0, device=device)
        m = np.asarray(mapping)
        if m.ndim != 1 or (len(m) and not np.issubdtype(m.dtype, np.integer)):
            raise ValueError("mapping must be a 1-d integer array (one block row per data row)")
        self.mapping = np.ascontiguousarray(m, np.int32)
        self.name = name

    def remap(self, mapping):
        """The same block (shared, on the device too) under another mapping."""
        return Relation(self.block, mapping, name=self.name)

    @property
    def size(self):
        return self.block.size


class RelationalData:
    """N labels, m >= 1 relations, an optional plain part (a ``DataSet`` or ``Features`` of the same N rows), ``batch_rows``.
    Feature ids are global and the parts' feature sets must be pairwise disjoint.  ``cache()`` moves it to the device
    (fmhip_relational_create); ``HipSGD.learn`` / ``step``, ``HipBlockMCMC.learn`` (and its ``test=``) and ``FMModel.predict`` /
    ``computeRMSE`` / ``computeLogLoss`` / ``computeAccuracy`` take it; every other call needs the flat rows: ``expand()``."""

    def __init__(self, y, relations, plain=None, batch_rows=0, name="relational", device=0):
        if isinstance(relations, Relation):
            relations = [relations]
        self.relations = list(relations)
        self.y = np.ascontiguousarray(y, np.float64)
        n = len(self.y)
        if self.y.ndim != 1:
            raise ValueError("y must be 1-d")
        if not self.relations:
            raise ValueError("a RelationalData needs at least one Relation")
        for i, rel in enumerate(self.relations):
            if not isinstance(rel, Relation):
                raise TypeError("relations must hold Relation objects, not %s" % type(rel).__name__)
            if len(rel.mapping) != n:
                raise ValueError("relation %d: the mapping holds %d entries, the data has %d rows" % (i, len(rel.mapping), n))
            bad = np.flatnonzero((rel.mapping < 0) | (rel.mapping >= rel.size))
            if len(bad):
                raise ValueError("relation %d: mapping[%d] = %d lies outside the block's rows [0, %d)" % (i, bad[0], rel.mapping[bad[0]], rel.size))
        self.name, self.device = name, int(device)
        br = int(batch_rows)
        self.batch_rows = br if 0 < br <= n else n
        self.plain = None
        if plain is not None:
            if plain.size != n:
                raise ValueError("the plain part has %d rows, the data %d" % (plain.size, n))
            own = isinstance(plain, DataSet) and (plain.batch_rows if 0 < plain.batch_rows <= n else n) == self.batch_rows
            # a DataSet batched as this one is taken as it stands; anything else is re-wrapped (the arrays are shared)
            self.plain = plain if own else DataSet(plain.row_ptr, plain.col, plain.val, self.y.astype(plain.val.dtype), name=name + ".plain",
                                                   batch_rows=self.batch_rows, device=self.device,
                                                   weights=getattr(plain, "weights", None), scoring=getattr(plain, "scoring", False))
        # an early answer on the host, as ValueError (the library checks both again at cache(): fmhip_relational_create)
        feats = [np.unique(part.col) for part in self._parts()]
        shared = [(int(both[0]), a, b) for b in range(len(feats)) for a in range(b) for both in [np.intersect1d(feats[a], feats[b], assume_unique=True)]
                  if len(both)]
        if shared:
            f, a, b = min(shared)
            raise ValueError("feature %d occurs in %s and in %s: the parts' feature sets must be disjoint" % (f, self._part_name(a), self._part_name(b)))
        self._h = None

    def _parts(self):
        return [rel.block for rel in self.relations] + ([self.plain] if self.plain is not None else [])

    def _part_name(self, p):
        return "relation %d" % p if p < len(self.relations) else "the plain part"

    # -- the DataSet surface the fit loop and the learners read ------------------------------
    @property
    def size(self):
        return len(self.y)

    @property
    def dimension(self):
        return max(part.dimension for part in self._parts())

    @property
    def n_batches(self):
        return (self.size + self.batch_rows - 1) // self.batch_rows if self.size else 0

    @property
    def targets(self):
        return self.y

    def cache(self):
        if self._h is None:
            L = _ffi.load()
            m = len(self.relations)
            blocks = (C.c_void_p * m)(*[rel.block.handle for rel in self.relations])
            maps = (C.c_void_p * m)(*[_ffi.ptr(rel.mapping) for rel in self.relations])
            h = C.c_void_p()
            _ffi.check(L.fmhip_relational_create(self.device, self.size, _ffi.ptr(self.y), m, blocks, maps,
                                                 None if self.plain is None else self.plain.handle, self.batch_rows, C.byref(h)))
            self._h = h
        return self

    def unpersist(self):
        """Frees the relational handle (the inverse maps, the workspace).  The blocks stay cached — other RelationalData may
        share them; they go with their Relation (``relation.block.unpersist()``), and must not go before this handle does."""
        if self._h is not None:
            _ffi.load().fmhip_relational_destroy(self._h)
            self._h = None
        return self

    def __del__(self):
        try:
            self.unpersist()
        except Exception:
            pass

    @property
    def rel_handle(self):
        return self.cache()._h

    @property
    def handle(self):
        raise TypeError("this call takes a flat DataSet, not a RelationalData (which HipSGD.learn / step, HipBlockMCMC.learn and FMModel.predict / computeRMSE / "
                        "computeLogLoss / computeAccuracy take): pass relational.expand()")

    def info(self):
        v = [C.c_int64() for _ in range(4)]
        m = C.c_int32()
        _ffi.check(_ffi.load().fmhip_relational_info(self.rel_handle, *[C.byref(x) for x in v], C.byref(m)))
        return dict(zip(("n_rows", "dimension", "batch_rows", "n_batches", "n_relations"), [int(x.value) for x in v] + [int(m.value)]))

    def expand(self):
        """The flat DataSet this stands for: per row relation 0's entries, then relation 1's, ..., then the plain part's."""
        n = self.size
        srcs = [(rel.block, rel.mapping.astype(np.int64)) for rel in self.relations]
        if self.plain is not None:
            srcs.append((self.plain, np.arange(n, dtype=np.int64)))
        lens = [blk.row_ptr[mp + 1] - blk.row_ptr[mp] for blk, mp in srcs]
        row_ptr = np.zeros(n + 1, np.int64)
        np.cumsum(np.sum(lens, axis=0), out=row_ptr[1:])
        col, val = np.empty(row_ptr[-1], np.int32), np.empty(row_ptr[-1], np.float64)
        at = row_ptr[:-1].copy()
        for (blk, mp), ln in zip(srcs, lens):
            within = np.arange(ln.sum(), dtype=np.int64) - np.repeat(np.cumsum(ln) - ln, ln)
            src, dst = np.repeat(blk.row_ptr[mp], ln) + within, np.repeat(at, ln) + within
            col[dst], val[dst] = blk.col[src], blk.val[src]
            at += ln
        return DataSet(row_ptr, col, val, self.y, name=self.name + ".flat", batch_rows=self.batch_rows, device=self.device)

    def meta(self):
        """The ``Metadata`` of the ``expand()``ed layout — a block is a group: the features relation 0's block uses are group 0,
        relation 1's group 1, ..., the plain part's the last; a feature id no part uses joins group 0.  What
        ``HipMCMC.run(groups=relational.meta())`` over ``relational.expand()`` takes."""
        from .metadata import Metadata
        parts = self._parts()
        groups = np.zeros(self.dimension, np.int32)
        for p, part in enumerate(parts):
            ids = np.unique(part.col)
            groups[ids[ids < self.dimension]] = p
        return Metadata(self.dimension).update(groups, numAttrGroups=len(parts))
