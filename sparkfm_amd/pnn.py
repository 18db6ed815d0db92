"""The product-based neural network (include/fmhip_pnn.h): a small multi-layer perceptron over the rows' concatenated field sums AND
their pairwise inner products (Qu et al., ICDM 2016, the inner-product form; the product layer is DLRM's dot interaction).  Entries of
one field are sum-pooled; the network's input is [s | g], g_p = <S_i, S_j> over the pairs i < j.

    train = FMUtils.loadLibFFMFile(path, batch_rows=65536)          # or FFMDataSet.from_rows(rows, y, batch_rows=256)
    model = PNN(train, 16, hidden=(64, 32)).learnWith(HipPNN.run(loss="logistic", optimizer="adagrad", eta=0.1, regv=1e-5, maxIteration=20))
    model.computeLogLoss(test), model.layers, model.u

The data is an FFMDataSet, unchanged.  A model and kernels of their own; there is no CPU fallback."""
import numpy as np

from .deepfm import DeepFMModel
from ._fieldmodel import FieldLearner


def pnn_width(num_fields, num_factor):
    """n_0 = F k + F (F - 1) / 2: the field sums, then the pairs i < j ascending in i, then in j."""
    return num_fields * num_factor + num_fields * (num_fields - 1) // 2


def pnn_init(seed, num_attribute, num_fields, num_factor, hidden, init_std=0.01):
    """(v, [(W_l, b_l)], u) drawn on the host from `seed` as deepfm_init draws them, W_1's fan-in n_0 = pnn_width(F, k)."""
    rng = np.random.default_rng(seed)
    v = rng.normal(0.0, init_std, (num_attribute + 1, num_factor))
    layers, fan = [], pnn_width(num_fields, num_factor)
    for n in hidden:
        a = np.sqrt(6.0 / fan)
        layers.append((rng.uniform(-a, a, (fan, n)), np.zeros(n)))
        fan = n
    a = np.sqrt(6.0 / fan)
    return v, layers, rng.uniform(-a, a, fan)


class PNNModel(DeepFMModel):
    """w0, w [n + 1], v [n + 1, k], the layers [(W_l [n_{l-1}, n_l], b_l [n_l])] with n_0 = F k + F (F - 1) / 2, and u [n_L] on the
    device (fmhip_pnn_model_t); get_params, set_params, layers, u, adagrad_state and set_adagrad_state as DeepFMModel's.  A new model
    is all zero, and an all-zero v has an all-zero gradient: PNN.learnWith draws v and the dense part."""

    _prefix = "fmhip_pnn"

    def _zeros(self):
        """(w, v, [W_l], [b_l], u) of zeros."""
        fans = (pnn_width(self.num_fields, self.num_factor),) + self.hidden[:-1]
        return (np.zeros(self.num_attribute + 1), np.zeros((self.num_attribute + 1, self.num_factor)),
                [np.zeros((a, b)) for a, b in zip(fans, self.hidden)], [np.zeros(b) for b in self.hidden], np.zeros(self.hidden[-1]))


class HipPNN(FieldLearner):
    """The PNN learner: mini-batch SGD or AdaGrad; v and w of the features a batch holds move, the dense part and w0 every batch.
    deep=False never steps the layers and u; linear=False never steps w0 and w."""

    _prefix, _flag, _reg = "fmhip_pnn", "deep", "regd"

    def __init__(self, loss="logistic", optimizer="adagrad", eta=0.1, reg0=0.0, regw=0.0, regv=1e-5, regd=0.0, linear=True, deep=True,
                 maxIteration=10, adagrad_eps=1e-10, adagrad_init=1.0):
        self._setup(loss, optimizer, eta, reg0, regw, regv, regd, linear, deep, maxIteration, adagrad_eps, adagrad_init)


class PNN:
    """PNN(train, k, hidden=(64, 32), seed=0, init_std=0.01).learnWith(HipPNN.run(...)) -> PNNModel, over an FFMDataSet."""

    def __init__(self, dataset, num_factor, hidden=(64, 32), seed=0, init_std=0.01, num_attribute=None, num_fields=None):
        self.dataset, self.num_factor, self.hidden = dataset, int(num_factor), tuple(int(n) for n in hidden)
        self.seed, self.init_std = int(seed), float(init_std)
        self.num_attribute = dataset.dimension if num_attribute is None else int(num_attribute)
        self.num_fields = dataset.num_fields if num_fields is None else int(num_fields)

    def learnWith(self, learner):
        model = PNNModel(self.num_attribute, self.num_fields, self.num_factor, self.hidden, device=self.dataset.device)
        v, layers, u = pnn_init(self.seed, self.num_attribute, self.num_fields, self.num_factor, self.hidden, self.init_std)
        model.set_params(0.0, np.zeros(self.num_attribute + 1), v, layers, u)
        return learner.fit(model, self.dataset)
