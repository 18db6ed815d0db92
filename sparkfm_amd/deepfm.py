"""DeepFM (include/fmhip_deepfm.h): the plain FM term plus a small multi-layer perceptron over the rows' concatenated field sums, both
reading the same feature embeddings (Guo et al., IJCAI 2017).  Entries of one field are sum-pooled into the MLP's input; the FM term is
the plain FM's over the row's entries.

    train = FMUtils.loadLibFFMFile(path, batch_rows=65536)          # or FFMDataSet.from_rows(rows, y, batch_rows=256)
    model = DeepFM(train, 16, hidden=(64, 32)).learnWith(HipDeepFM.run(loss="logistic", optimizer="adagrad", eta=0.1, regv=1e-5, maxIteration=20))
    model.computeLogLoss(test), model.layers, model.u

The data is an FFMDataSet, unchanged.  A model and kernels of their own; there is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _ffi
from ._fieldmodel import FieldLearner, FieldModel, pointers as _pointers


def deepfm_init(seed, num_attribute, num_fields, num_factor, hidden, init_std=0.01):
    """(v, [(W_l, b_l)], u) drawn on the host from `seed`: v ~ N(0, init_std^2), W_l and u He-uniform (U[-a, a], a = sqrt(6 / fan-in)),
    b_l = 0."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0.0, init_std, (num_attribute + 1, num_factor))
    layers, fan = [], num_fields * num_factor
    for n in hidden:
        a = np.sqrt(6.0 / fan)
        layers.append((rng.uniform(-a, a, (fan, n)), np.zeros(n)))
        fan = n
    a = np.sqrt(6.0 / fan)
    return v, layers, rng.uniform(-a, a, fan)


class DeepFMModel(FieldModel):
    """w0, w [n + 1], v [n + 1, k], the layers [(W_l [n_{l-1}, n_l], b_l [n_l])] with n_0 = F k, and u [n_L] on the device
    (fmhip_deepfm_model_t).  A new model is all zero, and an all-zero v has an all-zero gradient: DeepFM.learnWith draws v and the
    dense part."""

    _prefix, _info_tail = "fmhip_deepfm", 2

    def __init__(self, num_attribute, num_fields, num_factor, hidden=(64, 32), device=0, stream=None):
        self.hidden = tuple(int(n) for n in hidden)
        widths = np.array(self.hidden, np.int32)
        self._create(num_attribute, num_fields, num_factor, device, stream, len(self.hidden), widths.ctypes.data_as(C.POINTER(C.c_int32)))

    def _zeros(self):
        """(w, v, [W_l], [b_l], u) of zeros."""
        fans = (self.num_fields * self.num_factor,) + self.hidden[:-1]
        return (np.zeros(self.num_attribute + 1), np.zeros((self.num_attribute + 1, self.num_factor)),
                [np.zeros((a, b)) for a, b in zip(fans, self.hidden)], [np.zeros(b) for b in self.hidden], np.zeros(self.hidden[-1]))

    def _checked(self, prefix, w, v, layers, u):
        like = self._zeros()
        if len(layers) != len(self.hidden):
            raise ValueError("%slayers must hold %d (W, b) pairs, not %d" % (prefix, len(self.hidden), len(layers)))
        flat = [w, v] + [W for W, _ in layers] + [b for _, b in layers] + [u]
        names = ["w", "v"] + ["W_%d" % (l + 1) for l in range(len(layers))] + ["b_%d" % (l + 1) for l in range(len(layers))] + ["u"]
        out = [np.ascontiguousarray(x, np.float64) for x in flat]
        for name, x, z in zip(names, out, [like[0], like[1]] + like[2] + like[3] + [like[4]]):
            if x.shape != z.shape:
                raise ValueError("%s%s must have shape %r, not %r" % (prefix, name, z.shape, x.shape))
        L = len(layers)
        return out[0], out[1], out[2:2 + L], out[2 + L:2 + 2 * L], out[-1]

    def get_params(self):
        """(w0, w, v, layers, u), layers a list of (W_l, b_l)."""
        w0, (w, v, Ws, bs, u) = C.c_double(), self._zeros()
        self._call("model_get_params", self._h, C.byref(w0), _ffi.ptr(w), _ffi.ptr(v), _pointers(Ws), _pointers(bs), _ffi.ptr(u))
        return w0.value, w, v, list(zip(Ws, bs)), u

    def set_params(self, w0, w, v, layers, u):
        w, v, Ws, bs, u = self._checked("", w, v, layers, u)
        self._call("model_set_params", self._h, float(w0), _ffi.ptr(w), _ffi.ptr(v), _pointers(Ws), _pointers(bs), _ffi.ptr(u))

    w0 = property(lambda self: self.get_params()[0])
    w = property(lambda self: self.get_params()[1])
    v = property(lambda self: self.get_params()[2])
    layers = property(lambda self: self.get_params()[3])
    u = property(lambda self: self.get_params()[4])

    def adagrad_state(self):
        """(n0, nw, nv, [(nW_l, nb_l)], nu): AdaGrad's accumulators, shaped like the parameters (a model under SGD raises)."""
        n0, (nw, nv, Ws, bs, nu) = C.c_double(), self._zeros()
        self._call("model_get_accumulators", self._h, C.byref(n0), _ffi.ptr(nw), _ffi.ptr(nv), _pointers(Ws), _pointers(bs), _ffi.ptr(nu))
        return n0.value, nw, nv, list(zip(Ws, bs)), nu

    def set_adagrad_state(self, n0, nw, nv, nlayers, nu):
        nw, nv, Ws, bs, nu = self._checked("n", nw, nv, nlayers, nu)
        self._call("model_set_accumulators", self._h, float(n0), _ffi.ptr(nw), _ffi.ptr(nv), _pointers(Ws), _pointers(bs), _ffi.ptr(nu))


class HipDeepFM(FieldLearner):
    """The DeepFM learner: mini-batch SGD or AdaGrad; v and w of the features a batch holds move, the dense part and w0 every batch.
    deep=False never steps the layers and u (with u = 0: the plain FM); linear=False never steps w0 and w."""

    _prefix, _flag, _reg = "fmhip_deepfm", "deep", "regd"

    def __init__(self, loss="logistic", optimizer="adagrad", eta=0.1, reg0=0.0, regw=0.0, regv=1e-5, regd=0.0, linear=True, deep=True,
                 maxIteration=10, adagrad_eps=1e-10, adagrad_init=1.0):
        self._setup(loss, optimizer, eta, reg0, regw, regv, regd, linear, deep, maxIteration, adagrad_eps, adagrad_init)


class DeepFM:
    """DeepFM(train, k, hidden=(64, 32), seed=0, init_std=0.01).learnWith(HipDeepFM.run(...)) -> DeepFMModel, over an FFMDataSet."""

    def __init__(self, dataset, num_factor, hidden=(64, 32), seed=0, init_std=0.01, num_attribute=None, num_fields=None):
        self.dataset, self.num_factor, self.hidden = dataset, int(num_factor), tuple(int(n) for n in hidden)
        self.seed, self.init_std = int(seed), float(init_std)
        self.num_attribute = dataset.dimension if num_attribute is None else int(num_attribute)
        self.num_fields = dataset.num_fields if num_fields is None else int(num_fields)

    def learnWith(self, learner):
        model = DeepFMModel(self.num_attribute, self.num_fields, self.num_factor, self.hidden, device=self.dataset.device)
        v, layers, u = deepfm_init(self.seed, self.num_attribute, self.num_fields, self.num_factor, self.hidden, self.init_std)
        model.set_params(0.0, np.zeros(self.num_attribute + 1), v, layers, u)
        return learner.fit(model, self.dataset)
