"""AutoInt (include/fmhip_autoint.h): multi-head self-attention over the rows' field sums — each field attends to the other fields of
its own row —, X_{l+1} = relu(softmax(Q K^T) V + R) per head, scored as w0 + <w, x> + <vec(X_L), u> (Song et al., CIKM 2019).  Entries of
one field are sum-pooled into a token.

    train = FMUtils.loadLibFFMFile(path, batch_rows=65536)          # or FFMDataSet.from_rows(rows, y, batch_rows=256)
    model = AutoInt(train, 16, layers=2, heads=2, head_dim=16).learnWith(HipAutoInt.run(loss="logistic", optimizer="adagrad", eta=0.1, maxIteration=20))
    model.computeLogLoss(test), model.layers, model.u

The data is an FFMDataSet, unchanged.  A model and kernels of their own; there is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _ffi
from ._fieldmodel import FieldLearner, FieldModel, pointers as _pointers


def autoint_init(seed, num_attribute, num_fields, num_factor, layers, heads, head_dim, init_std=0.01):
    """(v, [W_l], u) drawn on the host from `seed`: v ~ N(0, init_std^2); W_l and u uniform with variance 1 / fan-in (U[-a, a],
    a = sqrt(3 / fan-in); fan-in D_l for W_l — k, then A = heads head_dim —, F A for u)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0.0, init_std, (num_attribute + 1, num_factor))
    A = heads * head_dim
    Ws = []
    for l in range(layers):
        D = num_factor if l == 0 else A
        Ws.append(rng.uniform(-1, 1, (D, 4 * A)) * np.sqrt(3.0 / D))
    return v, Ws, rng.uniform(-1, 1, num_fields * A) * np.sqrt(3.0 / (num_fields * A))


class AutoIntModel(FieldModel):
    """w0, w [n + 1], v [n + 1, k], the layers [W_l [D_l, 4A]] (D_0 = k, D_l = A = heads head_dim; W_l = [W_Q | W_K | W_V | W_R]) and
    u [F A] on the device (fmhip_autoint_model_t).  A new model is all zero, and an all-zero v has an all-zero gradient:
    AutoInt.learnWith draws v and the attention part."""

    _prefix, _info_tail = "fmhip_autoint", 3

    def __init__(self, num_attribute, num_fields, num_factor, layers=2, heads=2, head_dim=16, device=0, stream=None):
        self.n_layers, self.heads, self.head_dim = int(layers), int(heads), int(head_dim)
        self._create(num_attribute, num_fields, num_factor, device, stream, self.n_layers, self.heads, self.head_dim)

    def _zeros(self):
        """(w, v, [W_l], u) of zeros."""
        A = self.heads * self.head_dim
        return (np.zeros(self.num_attribute + 1), np.zeros((self.num_attribute + 1, self.num_factor)),
                [np.zeros((self.num_factor if l == 0 else A, 4 * A)) for l in range(self.n_layers)], np.zeros(self.num_fields * A))

    def _checked(self, prefix, w, v, layers, u):
        if len(layers) != self.n_layers:
            raise ValueError("%slayers must hold %d matrices, not %d" % (prefix, self.n_layers, len(layers)))
        like = self._zeros()
        names = ["w", "v"] + ["W_%d" % l for l in range(self.n_layers)] + ["u"]
        out = [np.ascontiguousarray(x, np.float64) for x in [w, v] + list(layers) + [u]]
        for name, x, z in zip(names, out, [like[0], like[1]] + like[2] + [like[3]]):
            if x.shape != z.shape:
                raise ValueError("%s%s must have shape %r, not %r" % (prefix, name, z.shape, x.shape))
        return out[0], out[1], out[2:-1], out[-1]

    def get_params(self):
        """(w0, w, v, layers, u), layers a list of W_l."""
        w0, (w, v, Ws, u) = C.c_double(), self._zeros()
        _ffi.check(_ffi.load().fmhip_autoint_model_get_params(self._h, C.byref(w0), _ffi.ptr(w), _ffi.ptr(v), _pointers(Ws), _ffi.ptr(u)))
        return w0.value, w, v, Ws, u

    def set_params(self, w0, w, v, layers, u):
        w, v, Ws, u = self._checked("", w, v, layers, u)
        _ffi.check(_ffi.load().fmhip_autoint_model_set_params(self._h, float(w0), _ffi.ptr(w), _ffi.ptr(v), _pointers(Ws), _ffi.ptr(u)))

    w0 = property(lambda self: self.get_params()[0])
    w = property(lambda self: self.get_params()[1])
    v = property(lambda self: self.get_params()[2])
    layers = property(lambda self: self.get_params()[3])
    u = property(lambda self: self.get_params()[4])

    def adagrad_state(self):
        """(n0, nw, nv, [nW_l], nu): AdaGrad's accumulators, shaped like the parameters (a model under SGD raises)."""
        n0, (nw, nv, Ws, nu) = C.c_double(), self._zeros()
        _ffi.check(_ffi.load().fmhip_autoint_model_get_accumulators(self._h, C.byref(n0), _ffi.ptr(nw), _ffi.ptr(nv), _pointers(Ws), _ffi.ptr(nu)))
        return n0.value, nw, nv, Ws, nu

    def set_adagrad_state(self, n0, nw, nv, nlayers, nu):
        nw, nv, Ws, nu = self._checked("n", nw, nv, nlayers, nu)
        _ffi.check(_ffi.load().fmhip_autoint_model_set_accumulators(self._h, float(n0), _ffi.ptr(nw), _ffi.ptr(nv), _pointers(Ws), _ffi.ptr(nu)))


class HipAutoInt(FieldLearner):
    """The AutoInt learner: mini-batch SGD or AdaGrad; v and w of the features a batch holds move, the attention part and w0 every
    batch.  attention=False never steps W_l and u; linear=False never steps w0 and w."""

    _prefix, _flag, _reg = "fmhip_autoint", "attention", "regd"

    def __init__(self, loss="logistic", optimizer="adagrad", eta=0.1, reg0=0.0, regw=0.0, regv=1e-5, regd=0.0, linear=True, attention=True,
                 maxIteration=10, adagrad_eps=1e-10, adagrad_init=1.0):
        self._setup(loss, optimizer, eta, reg0, regw, regv, regd, linear, attention, maxIteration, adagrad_eps, adagrad_init)


class AutoInt:
    """AutoInt(train, k, layers=2, heads=2, head_dim=16, seed=0, init_std=0.01).learnWith(HipAutoInt.run(...)) -> AutoIntModel, over an
    FFMDataSet."""

    def __init__(self, dataset, num_factor, layers=2, heads=2, head_dim=16, seed=0, init_std=0.01, num_attribute=None, num_fields=None):
        self.dataset, self.num_factor, self.layers, self.heads, self.head_dim = dataset, int(num_factor), int(layers), int(heads), int(head_dim)
        self.seed, self.init_std = int(seed), float(init_std)
        self.num_attribute = dataset.dimension if num_attribute is None else int(num_attribute)
        self.num_fields = dataset.num_fields if num_fields is None else int(num_fields)

    def learnWith(self, learner):
        model = AutoIntModel(self.num_attribute, self.num_fields, self.num_factor, self.layers, self.heads, self.head_dim, device=self.dataset.device)
        v, Ws, u = autoint_init(self.seed, self.num_attribute, self.num_fields, self.num_factor, self.layers, self.heads, self.head_dim, self.init_std)
        model.set_params(0.0, np.zeros(self.num_attribute + 1), v, Ws, u)
        return learner.fit(model, self.dataset)
