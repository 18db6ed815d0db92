"""DCN-V2's low-rank cross network (include/fmhip_dcn.h): explicit feature crosses of degree up to L + 1 over the rows' concatenated
field sums, x_{l+1} = x_0 o (x_l V_l U_l + c_l) + x_l, scored as w0 + <w, x> + <x_L, u> (Wang et al., WWW 2021).  Entries of one field
are sum-pooled into x_0.

    train = FMUtils.loadLibFFMFile(path, batch_rows=65536)          # or FFMDataSet.from_rows(rows, y, batch_rows=256)
    model = DCN(train, 16, cross_layers=2, rank=64).learnWith(HipDCN.run(loss="logistic", optimizer="adagrad", eta=0.1, regv=1e-5, maxIteration=20))
    model.computeLogLoss(test), model.cross, model.u

The data is an FFMDataSet, unchanged.  A model and kernels of their own; there is no CPU fallback."""
import ctypes as C

import numpy as np

from . import _ffi
from ._fieldmodel import FieldLearner, FieldModel, pointers as _pointers


def dcn_init(seed, num_attribute, num_fields, num_factor, cross_layers, rank, init_std=0.01):
    """(v, [(V_l, U_l, c_l)], u) drawn on the host from `seed`: v ~ N(0, init_std^2); V_l, U_l and u uniform with variance 1 / fan-in
    (U[-a, a], a = sqrt(3 / fan-in); fan-in P = F k for V_l and u, rank for U_l); c_l = 0."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0.0, init_std, (num_attribute + 1, num_factor))
    P = num_fields * num_factor
    aP, ar = np.sqrt(3.0 / P), np.sqrt(3.0 / rank)
    cross = [(rng.uniform(-aP, aP, (P, rank)), rng.uniform(-ar, ar, (rank, P)), np.zeros(P)) for _ in range(cross_layers)]
    return v, cross, rng.uniform(-aP, aP, P)


class DCNModel(FieldModel):
    """w0, w [n + 1], v [n + 1, k], the cross layers [(V_l [F k, r], U_l [r, F k], c_l [F k])] and u [F k] on the device
    (fmhip_dcn_model_t).  A new model is all zero, and an all-zero v has an all-zero gradient: DCN.learnWith draws v and the cross part."""

    _prefix, _info_tail = "fmhip_dcn", 2

    def __init__(self, num_attribute, num_fields, num_factor, cross_layers=2, rank=64, device=0, stream=None):
        self.cross_layers, self.rank = int(cross_layers), int(rank)
        self._create(num_attribute, num_fields, num_factor, device, stream, self.cross_layers, self.rank)

    def _zeros(self):
        """(w, v, [V_l], [U_l], [c_l], u) of zeros."""
        P, r, L = self.num_fields * self.num_factor, self.rank, range(self.cross_layers)
        return (np.zeros(self.num_attribute + 1), np.zeros((self.num_attribute + 1, self.num_factor)),
                [np.zeros((P, r)) for _ in L], [np.zeros((r, P)) for _ in L], [np.zeros(P) for _ in L], np.zeros(P))

    def _checked(self, prefix, w, v, cross, u):
        L = self.cross_layers
        if len(cross) != L:
            raise ValueError("%scross must hold %d (V, U, c) triples, not %d" % (prefix, L, len(cross)))
        like = self._zeros()
        flat = [w, v] + [t[0] for t in cross] + [t[1] for t in cross] + [t[2] for t in cross] + [u]
        names = ["w", "v"] + ["%s_%d" % (s, l) for s in "VUc" for l in range(L)] + ["u"]
        out = [np.ascontiguousarray(x, np.float64) for x in flat]
        for name, x, z in zip(names, out, [like[0], like[1]] + like[2] + like[3] + like[4] + [like[5]]):
            if x.shape != z.shape:
                raise ValueError("%s%s must have shape %r, not %r" % (prefix, name, z.shape, x.shape))
        return out[0], out[1], out[2:2 + L], out[2 + L:2 + 2 * L], out[2 + 2 * L:2 + 3 * L], out[-1]

    def get_params(self):
        """(w0, w, v, cross, u), cross a list of (V_l, U_l, c_l)."""
        w0, (w, v, Vs, Us, cs, u) = C.c_double(), self._zeros()
        _ffi.check(_ffi.load().fmhip_dcn_model_get_params(self._h, C.byref(w0), _ffi.ptr(w), _ffi.ptr(v), _pointers(Vs), _pointers(Us), _pointers(cs),
                                                          _ffi.ptr(u)))
        return w0.value, w, v, list(zip(Vs, Us, cs)), u

    def set_params(self, w0, w, v, cross, u):
        w, v, Vs, Us, cs, u = self._checked("", w, v, cross, u)
        _ffi.check(_ffi.load().fmhip_dcn_model_set_params(self._h, float(w0), _ffi.ptr(w), _ffi.ptr(v), _pointers(Vs), _pointers(Us), _pointers(cs),
                                                          _ffi.ptr(u)))

    w0 = property(lambda self: self.get_params()[0])
    w = property(lambda self: self.get_params()[1])
    v = property(lambda self: self.get_params()[2])
    cross = property(lambda self: self.get_params()[3])
    u = property(lambda self: self.get_params()[4])

    def adagrad_state(self):
        """(n0, nw, nv, [(nV_l, nU_l, nc_l)], nu): AdaGrad's accumulators, shaped like the parameters (a model under SGD raises)."""
        n0, (nw, nv, Vs, Us, cs, nu) = C.c_double(), self._zeros()
        _ffi.check(_ffi.load().fmhip_dcn_model_get_accumulators(self._h, C.byref(n0), _ffi.ptr(nw), _ffi.ptr(nv), _pointers(Vs), _pointers(Us),
                                                                _pointers(cs), _ffi.ptr(nu)))
        return n0.value, nw, nv, list(zip(Vs, Us, cs)), nu

    def set_adagrad_state(self, n0, nw, nv, ncross, nu):
        nw, nv, Vs, Us, cs, nu = self._checked("n", nw, nv, ncross, nu)
        _ffi.check(_ffi.load().fmhip_dcn_model_set_accumulators(self._h, float(n0), _ffi.ptr(nw), _ffi.ptr(nv), _pointers(Vs), _pointers(Us),
                                                                _pointers(cs), _ffi.ptr(nu)))


class HipDCN(FieldLearner):
    """The DCN-V2 learner: mini-batch SGD or AdaGrad; v and w of the features a batch holds move, the cross part and w0 every batch.
    cross=False never steps V_l, U_l, c_l and u; linear=False never steps w0 and w."""

    _prefix, _flag, _reg = "fmhip_dcn", "cross", "regd"

    def __init__(self, loss="logistic", optimizer="adagrad", eta=0.1, reg0=0.0, regw=0.0, regv=1e-5, regd=0.0, linear=True, cross=True,
                 maxIteration=10, adagrad_eps=1e-10, adagrad_init=1.0):
        self._setup(loss, optimizer, eta, reg0, regw, regv, regd, linear, cross, maxIteration, adagrad_eps, adagrad_init)


class DCN:
    """DCN(train, k, cross_layers=2, rank=64, seed=0, init_std=0.01).learnWith(HipDCN.run(...)) -> DCNModel, over an FFMDataSet."""

    def __init__(self, dataset, num_factor, cross_layers=2, rank=64, seed=0, init_std=0.01, num_attribute=None, num_fields=None):
        self.dataset, self.num_factor, self.cross_layers, self.rank = dataset, int(num_factor), int(cross_layers), int(rank)
        self.seed, self.init_std = int(seed), float(init_std)
        self.num_attribute = dataset.dimension if num_attribute is None else int(num_attribute)
        self.num_fields = dataset.num_fields if num_fields is None else int(num_fields)

    def learnWith(self, learner):
        model = DCNModel(self.num_attribute, self.num_fields, self.num_factor, self.cross_layers, self.rank, device=self.dataset.device)
        v, cross, u = dcn_init(self.seed, self.num_attribute, self.num_fields, self.num_factor, self.cross_layers, self.rank, self.init_std)
        model.set_params(0.0, np.zeros(self.num_attribute + 1), v, cross, u)
        return learner.fit(model, self.dataset)
