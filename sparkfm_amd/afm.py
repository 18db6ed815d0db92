"""The Attentional Factorization Machine (include/fmhip_afm.h): every pair of fields interacts through E_ij = S_i o S_j, a net with one
hidden layer of t units scores each product per row, s_ij = <h, relu(W E_ij + b)>, a softmax over the pairs weights them, and the
margin is w0 + <w, x> + <p, sum_ij a_ij E_ij> (Xiao et al., IJCAI 2017).  Entries of one field are sum-pooled into S.

    train = FMUtils.loadLibFFMFile(path, batch_rows=65536)          # or FFMDataSet.from_rows(rows, y, batch_rows=256)
    model = AFM(train, 16, attention_factor=32).learnWith(HipAFM.run(loss="logistic", optimizer="adagrad", eta=0.1, regv=1e-5, maxIteration=20))
    model.computeLogLoss(test), model.W, model.p

The data is an FFMDataSet, unchanged.  A model and kernels of their own; there is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _ffi
from ._fieldmodel import FieldLearner, FieldModel


def afm_init(seed, num_attribute, num_factor, attention_factor, init_std=0.01):
    """(v, W, b, h, p) drawn on the host from `seed`: v ~ N(0, init_std^2); W, h and p uniform with variance 1 / fan-in (U[-a, a],
    a = sqrt(3 / fan-in); fan-in k for W and p, t for h); b = 0."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0.0, init_std, (num_attribute + 1, num_factor))
    a, at = np.sqrt(3.0 / num_factor), np.sqrt(3.0 / attention_factor)
    W = rng.uniform(-a, a, (attention_factor, num_factor))
    h = rng.uniform(-at, at, attention_factor)
    return v, W, np.zeros(attention_factor), h, rng.uniform(-a, a, num_factor)


class AFMModel(FieldModel):
    """w0, w [n + 1], v [n + 1, k], W [t, k], b [t], h [t] and p [k] on the device (fmhip_afm_model_t).  A new model is all zero, and an
    all-zero v has an all-zero gradient: AFM.learnWith draws v and the attention part."""

    _prefix, _info_tail = "fmhip_afm", 1

    def __init__(self, num_attribute, num_fields, num_factor, attention_factor=32, device=0, stream=None):
        self.attention_factor = int(attention_factor)
        self._create(num_attribute, num_fields, num_factor, device, stream, self.attention_factor)

    def _zeros(self):
        """(w, v, W, b, h, p) of zeros."""
        n1, k, t = self.num_attribute + 1, self.num_factor, self.attention_factor
        return np.zeros(n1), np.zeros((n1, k)), np.zeros((t, k)), np.zeros(t), np.zeros(t), np.zeros(k)

    def _checked(self, prefix, *arrays):
        out = [np.ascontiguousarray(x, np.float64) for x in arrays]
        for name, x, z in zip(("w", "v", "W", "b", "h", "p"), out, self._zeros()):
            if x.shape != z.shape:
                raise ValueError("%s%s must have shape %r, not %r" % (prefix, name, z.shape, x.shape))
        return out

    def get_params(self):
        """(w0, w, v, W, b, h, p)."""
        w0, out = C.c_double(), self._zeros()
        self._call("model_get_params", self._h, C.byref(w0), *[_ffi.ptr(x) for x in out])
        return (w0.value,) + out

    def set_params(self, w0, w, v, W, b, h, p):
        self._call("model_set_params", self._h, float(w0), *[_ffi.ptr(x) for x in self._checked("", w, v, W, b, h, p)])

    w0 = property(lambda self: self.get_params()[0])
    w = property(lambda self: self.get_params()[1])
    v = property(lambda self: self.get_params()[2])
    W = property(lambda self: self.get_params()[3])
    b = property(lambda self: self.get_params()[4])
    h = property(lambda self: self.get_params()[5])
    p = property(lambda self: self.get_params()[6])

    def adagrad_state(self):
        """(n0, nw, nv, nW, nb, nh, np): AdaGrad's accumulators, shaped like the parameters (a model under SGD raises)."""
        n0, out = C.c_double(), self._zeros()
        self._call("model_get_accumulators", self._h, C.byref(n0), *[_ffi.ptr(x) for x in out])
        return (n0.value,) + out

    def set_adagrad_state(self, n0, nw, nv, nW, nb, nh, np_):
        self._call("model_set_accumulators", self._h, float(n0), *[_ffi.ptr(x) for x in self._checked("n", nw, nv, nW, nb, nh, np_)])


class HipAFM(FieldLearner):
    """The AFM learner: mini-batch SGD or AdaGrad; v and w of the features a batch holds move, the attention part and w0 every batch.
    attention=False never steps W, b, h and p; linear=False never steps w0 and w."""

    _prefix, _flag, _reg = "fmhip_afm", "attention", "regd"

    def __init__(self, loss="logistic", optimizer="adagrad", eta=0.1, reg0=0.0, regw=0.0, regv=1e-5, regd=0.0, linear=True, attention=True,
                 maxIteration=10, adagrad_eps=1e-10, adagrad_init=1.0):
        self._setup(loss, optimizer, eta, reg0, regw, regv, regd, linear, attention, maxIteration, adagrad_eps, adagrad_init)


class AFM:
    """AFM(train, k, attention_factor=32, seed=0, init_std=0.01).learnWith(HipAFM.run(...)) -> AFMModel, over an FFMDataSet."""

    def __init__(self, dataset, num_factor, attention_factor=32, seed=0, init_std=0.01, num_attribute=None, num_fields=None):
        self.dataset, self.num_factor, self.attention_factor = dataset, int(num_factor), int(attention_factor)
        self.seed, self.init_std = int(seed), float(init_std)
        self.num_attribute = dataset.dimension if num_attribute is None else int(num_attribute)
        self.num_fields = dataset.num_fields if num_fields is None else int(num_fields)

    def learnWith(self, learner):
        model = AFMModel(self.num_attribute, self.num_fields, self.num_factor, self.attention_factor, device=self.dataset.device)
        v, W, b, h, p = afm_init(self.seed, self.num_attribute, self.num_factor, self.attention_factor, self.init_std)
        model.set_params(0.0, np.zeros(self.num_attribute + 1), v, W, b, h, p)
        return learner.fit(model, self.dataset)
