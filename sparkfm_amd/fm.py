"""FM façade + fit loop — host mirror of S/fm/FM.scala and S/fm/impl/FactorizationMachines.scala."""
import logging

from .model import FMModel
from .relational import Relation, RelationalData

log = logging.getLogger("sparkfm_amd")


class Task:
    """S/Task.scala:3-6 (accepted and, as in the reference, never read).  The loss is the learner's: a binary
    classifier is ``FM(dataset, k).learnWith(HipSGD.run(loss="logistic"))`` (labels {0,1} or {-1,+1}), scored by
    ``fm.computeLogLoss(test)`` and ``fm.computeAccuracy(test)``; a ranking model is
    ``FM(DataSet.from_pairs(preferred, other), k).learnWith(HipSGD.run(loss="logistic", pairs=True))``, scored by
    ``fm.computePairLogLoss(test)`` and ``fm.computePairAccuracy(test)``."""
    Regression = "Regression"
    Classification = "Classification"


class FactorizationMachines:
    """S/fm/impl/FactorizationMachines.scala:9-53."""

    def __init__(self, dataset, numFactor=8, task=Task.Regression, maxIteration=100, timeout=0, seed=0):
        self.dataset = dataset
        self.numFactor = numFactor
        self.task = task
        self.maxIteration = maxIteration
        self.timeout = timeout
        self.seed = seed
        self.rmse_history = []
        self.relations = []

    def withRelation(self, relation):
        """S/fm/impl/FactorizationMachines.scala:24-28: appends a Relation (or each of a list) and returns self.  The reference's
        S/fm/bs/* is a stub; here the relations train as block-structure FM: `learnWith` fits
        RelationalData(dataset.y, relations, plain = dataset if it has nonzeros), batched as `dataset`."""
        for rel in ([relation] if isinstance(relation, Relation) else list(relation)):
            if not isinstance(rel, Relation):
                raise TypeError("withRelation takes a Relation or a list of them, not %s" % type(rel).__name__)
            self.relations.append(rel)
        return self

    def learnWith(self, fml, init=None):
        """S/fm/impl/FactorizationMachines.scala:30-51: cache; new FMModel(dimension, numFactor);
        maxIteration x { computeRMSE (logged); fm = fml.learn(fm, dataset) }; unpersist.
        `init` = (w0, w, v) injects parameters (the reference's own init is unseeded, quirk Q2).  A learner that trains on more
        than `dataset` says so through a `dimension` of its own (``HipBPR``: the larger of its two blocks'): the model holds both."""
        ds = self.dataset
        if self.relations:
            ds = RelationalData(ds.y, self.relations, plain=ds if ds.nnz else None, batch_rows=ds.batch_rows, name=ds.name, device=ds.device)
        ds = ds.cache()                                               # :36
        fm = FMModel(max(ds.dimension, getattr(fml, "dimension", 0)), self.numFactor, seed=self.seed, device=ds.device)   # :39
        if init is not None:
            fm.w0, fm.w, fm.v = init
        for i in range(1, self.maxIteration + 1):                     # :42
            rmse = fm.computeRMSE(ds)                                 # :43
            self.rmse_history.append(rmse)
            log.info("Iteration %d in progress... (%s RMSE = %.6f)", i, ds.name, rmse)
            fm = fml.learn(fm, ds)                                    # :45
        ds.unpersist()                                                # :48
        if ds is not self.dataset and ds.plain is not None:
            # the relational handle is gone: the plain part leaves the device as the flat fit's dataset does; the blocks stay cached
            # with their Relation, which other fits and held-out data may share (relation.block.unpersist())
            ds.plain.unpersist()
        return fm


def FM(dataset, numFactor, task=Task.Regression, maxIteration=100, timeout=0, seed=0):
    """FM.apply (S/fm/FM.scala:25-33)."""
    return FactorizationMachines(dataset, numFactor, task, maxIteration, timeout, seed)
