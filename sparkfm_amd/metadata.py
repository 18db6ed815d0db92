"""Attribute groups: which feature belongs to which group (users, items, a context field, a bag of words ...).

``Metadata(dimension)`` follows the reference's ``fm/bs/Metadata.scala`` — ``attrGroup``, ``numAttrGroups``, ``numAttrPerGroup``,
``update(groups)`` — and is what ``HipMCMC.run(groups=...)`` takes: the MCMC learner then samples a regulariser lambda and a prior
mean mu per (parameter group, attribute group) (include/fmhip_mcmc_groups.h).

One departure, recorded in DESIGN.md: the reference's ``reload`` takes ``groups.max`` as the number of groups, which is one short
for 0-based ids — its own per-group write then runs off the end of the array.  Here the count is ``max + 1``.
"""
import numpy as np


class Metadata:
    def __init__(self, dimension):
        import operator
        dimension = operator.index(dimension)
        if dimension < 0:
            raise ValueError("dimension must be >= 0, not %d" % dimension)
        self.dimension = dimension
        self._attrGroup = np.zeros(dimension, np.int32)
        self._numAttrGroups = 1
        self._numAttrPerGroup = np.full(1, dimension, np.int64)

    @property
    def attrGroup(self):
        """int32 [dimension]: feature i's group."""
        return self._attrGroup

    @property
    def numAttrGroups(self):
        return self._numAttrGroups

    @property
    def numAttrPerGroup(self):
        """int64 [numAttrGroups]: how many features each group holds (0 for a group no feature names)."""
        return self._numAttrPerGroup

    def update(self, groups, numAttrGroups=None):
        """Replaces the table: `groups` holds one id >= 0 per feature (`dimension` of them); the count is max + 1 unless
        `numAttrGroups` asks for more (trailing groups without a feature)."""
        g = np.asarray(groups)
        if g.ndim != 1 or len(g) != self.dimension:
            raise ValueError("groups must hold one id per feature: %d, not an array of shape %s" % (self.dimension, g.shape))
        if len(g) and not np.issubdtype(g.dtype, np.integer):
            raise TypeError("group ids must be integers, not %s" % g.dtype)
        if len(g) and g.min() < 0:
            raise ValueError("feature %d has group id %d: ids are >= 0" % (int(np.argmin(g)), int(g.min())))
        n = int(g.max()) + 1 if len(g) else 1
        if numAttrGroups is not None:
            if int(numAttrGroups) < n:
                raise ValueError("numAttrGroups = %d but the table names group %d" % (int(numAttrGroups), n - 1))
            n = int(numAttrGroups)
        self._attrGroup = np.ascontiguousarray(g, np.int32)
        self._numAttrGroups = n
        self._numAttrPerGroup = np.bincount(self._attrGroup, minlength=n).astype(np.int64)
        return self

    @classmethod
    def fromFields(cls, sizes, dimension=None):
        """Contiguous fields: the first sizes[0] features are group 0, the next sizes[1] group 1, ...  `dimension` (default: their
        sum) may be larger — the features behind the last field join the last group."""
        sizes = [int(s) for s in sizes]
        if not sizes or min(sizes) < 0:
            raise ValueError("sizes must hold at least one field size, each >= 0")
        total = sum(sizes)
        dimension = total if dimension is None else int(dimension)
        if dimension < total:
            raise ValueError("the fields hold %d features, more than dimension = %d" % (total, dimension))
        groups = np.repeat(np.arange(len(sizes), dtype=np.int32), sizes)
        groups = np.concatenate([groups, np.full(dimension - total, len(sizes) - 1, np.int32)])
        return cls(dimension).update(groups, numAttrGroups=len(sizes))
