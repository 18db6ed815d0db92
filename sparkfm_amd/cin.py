"""xDeepFM's Compressed Interaction Network (include/fmhip_cin.h): explicit feature crosses of degree up to L + 1 over the rows' field
sums, formed vector-wise — X^l[h] = sum_{i,j} W_l[h, i, j] X^{l-1}[i] o X^0[j], p^l = the maps' sums over the k dimensions — and scored
as w0 + <w, x> + <[p^1 .. p^L], u> (Lian et al., KDD 2018).  Entries of one field are sum-pooled into X^0.

    train = FMUtils.loadLibFFMFile(path, batch_rows=65536)          # or FFMDataSet.from_rows(rows, y, batch_rows=256)
    model = CIN(train, 16, feature_maps=(32, 32)).learnWith(HipCIN.run(loss="logistic", optimizer="adagrad", eta=0.1, regv=1e-5, maxIteration=20))
    model.computeLogLoss(test), model.layers, model.u

The data is an FFMDataSet, unchanged.  A model and kernels of their own; there is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _ffi
from ._fieldmodel import FieldLearner, FieldModel, pointers as _pointers


def cin_init(seed, num_attribute, num_fields, num_factor, feature_maps, init_std=0.01):
    """(v, [W_l], u) drawn on the host from `seed`: v ~ N(0, init_std^2); W_l and u uniform with variance 1 / fan-in (U[-a, a],
    a = sqrt(3 / fan-in); fan-in H_{l-1} F for W_l, sum_l H_l for u)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0.0, init_std, (num_attribute + 1, num_factor))
    layers, prev = [], num_fields
    for h in feature_maps:
        a = np.sqrt(3.0 / (prev * num_fields))
        layers.append(rng.uniform(-a, a, (h, prev, num_fields)))
        prev = h
    a = np.sqrt(3.0 / sum(feature_maps))
    return v, layers, rng.uniform(-a, a, sum(feature_maps))


class CINModel(FieldModel):
    """w0, w [n + 1], v [n + 1, k], the layers [W_l [H_l, H_{l-1}, F]] with H_0 = F, and u [H_1 + .. + H_L] on the device
    (fmhip_cin_model_t).  A new model is all zero, and an all-zero v has an all-zero gradient: CIN.learnWith draws v and the CIN part."""

    _prefix, _info_tail = "fmhip_cin", 2

    def __init__(self, num_attribute, num_fields, num_factor, feature_maps=(32, 32), device=0, stream=None):
        self.feature_maps = tuple(int(h) for h in feature_maps)
        maps = np.array(self.feature_maps, np.int32)
        self._create(num_attribute, num_fields, num_factor, device, stream, len(self.feature_maps), maps.ctypes.data_as(C.POINTER(C.c_int32)))

    def _zeros(self):
        """(w, v, [W_l], u) of zeros."""
        prev = (self.num_fields,) + self.feature_maps[:-1]
        return (np.zeros(self.num_attribute + 1), np.zeros((self.num_attribute + 1, self.num_factor)),
                [np.zeros((h, p, self.num_fields)) for h, p in zip(self.feature_maps, prev)], np.zeros(sum(self.feature_maps)))

    def _checked(self, prefix, w, v, layers, u):
        like = self._zeros()
        if len(layers) != len(self.feature_maps):
            raise ValueError("%slayers must hold %d arrays W_l, not %d" % (prefix, len(self.feature_maps), len(layers)))
        names = ["w", "v"] + ["W_%d" % (l + 1) for l in range(len(layers))] + ["u"]
        out = [np.ascontiguousarray(x, np.float64) for x in [w, v] + list(layers) + [u]]
        for name, x, z in zip(names, out, [like[0], like[1]] + like[2] + [like[3]]):
            if x.shape != z.shape:
                raise ValueError("%s%s must have shape %r, not %r" % (prefix, name, z.shape, x.shape))
        return out[0], out[1], out[2:-1], out[-1]

    def get_params(self):
        """(w0, w, v, layers, u), layers a list of W_l."""
        w0, (w, v, Ws, u) = C.c_double(), self._zeros()
        _ffi.check(_ffi.load().fmhip_cin_model_get_params(self._h, C.byref(w0), _ffi.ptr(w), _ffi.ptr(v), _pointers(Ws), _ffi.ptr(u)))
        return w0.value, w, v, Ws, u

    def set_params(self, w0, w, v, layers, u):
        w, v, Ws, u = self._checked("", w, v, layers, u)
        _ffi.check(_ffi.load().fmhip_cin_model_set_params(self._h, float(w0), _ffi.ptr(w), _ffi.ptr(v), _pointers(Ws), _ffi.ptr(u)))

    w0 = property(lambda self: self.get_params()[0])
    w = property(lambda self: self.get_params()[1])
    v = property(lambda self: self.get_params()[2])
    layers = property(lambda self: self.get_params()[3])
    u = property(lambda self: self.get_params()[4])

    def adagrad_state(self):
        """(n0, nw, nv, [nW_l], nu): AdaGrad's accumulators, shaped like the parameters (a model under SGD raises)."""
        n0, (nw, nv, Ws, nu) = C.c_double(), self._zeros()
        _ffi.check(_ffi.load().fmhip_cin_model_get_accumulators(self._h, C.byref(n0), _ffi.ptr(nw), _ffi.ptr(nv), _pointers(Ws), _ffi.ptr(nu)))
        return n0.value, nw, nv, Ws, nu

    def set_adagrad_state(self, n0, nw, nv, nlayers, nu):
        nw, nv, Ws, nu = self._checked("n", nw, nv, nlayers, nu)
        _ffi.check(_ffi.load().fmhip_cin_model_set_accumulators(self._h, float(n0), _ffi.ptr(nw), _ffi.ptr(nv), _pointers(Ws), _ffi.ptr(nu)))


class HipCIN(FieldLearner):
    """The CIN learner: mini-batch SGD or AdaGrad; v and w of the features a batch holds move, the CIN part and w0 every batch.
    cin=False never steps W_l and u; linear=False never steps w0 and w."""

    _prefix, _flag, _reg = "fmhip_cin", "cin", "regd"

    def __init__(self, loss="logistic", optimizer="adagrad", eta=0.1, reg0=0.0, regw=0.0, regv=1e-5, regd=0.0, linear=True, cin=True,
                 maxIteration=10, adagrad_eps=1e-10, adagrad_init=1.0):
        self._setup(loss, optimizer, eta, reg0, regw, regv, regd, linear, cin, maxIteration, adagrad_eps, adagrad_init)


class CIN:
    """CIN(train, k, feature_maps=(32, 32), seed=0, init_std=0.01).learnWith(HipCIN.run(...)) -> CINModel, over an FFMDataSet."""

    def __init__(self, dataset, num_factor, feature_maps=(32, 32), seed=0, init_std=0.01, num_attribute=None, num_fields=None):
        self.dataset, self.num_factor, self.feature_maps = dataset, int(num_factor), tuple(int(h) for h in feature_maps)
        self.seed, self.init_std = int(seed), float(init_std)
        self.num_attribute = dataset.dimension if num_attribute is None else int(num_attribute)
        self.num_fields = dataset.num_fields if num_fields is None else int(num_fields)

    def learnWith(self, learner):
        model = CINModel(self.num_attribute, self.num_fields, self.num_factor, self.feature_maps, device=self.dataset.device)
        v, layers, u = cin_init(self.seed, self.num_attribute, self.num_fields, self.num_factor, self.feature_maps, self.init_std)
        model.set_params(0.0, np.zeros(self.num_attribute + 1), v, layers, u)
        return learner.fit(model, self.dataset)
