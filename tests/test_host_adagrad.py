"""AdaGrad without a GPU: the C ABI's argument checks (fmhip_model_set_optimizer and the state I/O of fmhip_experimental.h),
the Python learners' `optimizer=` validation, and the tests' own fp64 rule (train_ref.py) pinned to torch.optim.Adagrad."""
import ctypes as C
import math

import numpy as np
import pytest

from train_ref import adagrad_rule


def L():
    from sparkfm_amd import _ffi
    return _ffi.load()


def test_optimizer_entry_points_are_exported_and_bound():
    from sparkfm_amd import _ffi
    assert "fmhip_model_set_optimizer" in _ffi.SYMBOLS
    assert {"fmhip_model_get_optimizer_state", "fmhip_model_set_optimizer_state"} <= set(_ffi.SYMBOLS_EXPERIMENTAL)
    lib = L()
    for name in ("fmhip_model_set_optimizer", "fmhip_model_get_optimizer_state", "fmhip_model_set_optimizer_state"):
        assert hasattr(lib, name)
    assert (_ffi.OPT_SGD, _ffi.OPT_ADAGRAD) == (0, 1)


@pytest.mark.parametrize("opt,eps,init", [(2, 1e-10, 0.1), (-1, 1e-10, 0.1), (1, 0.0, 0.1), (1, -1e-10, 0.1), (1, math.inf, 0.1),
                                          (1, math.nan, 0.1), (1, 1e-10, -0.1), (1, 1e-10, math.inf), (1, 1e-10, math.nan)])
def test_set_optimizer_refuses_bad_values(opt, eps, init):
    """An unknown optimizer, eps not finite or <= 0, an initial accumulator not finite or < 0: FMHIP_ERR_INVALID (checked
    before the model, so a NULL model gets the same answer) and a message naming what is wrong."""
    from sparkfm_amd import _ffi
    assert L().fmhip_model_set_optimizer(None, opt, eps, init) == -1
    msg = L().fmhip_last_error().decode()
    assert ("optimizer" in msg) or ("eps" in msg) or ("initial_accumulator" in msg), msg
    assert _ffi.OPT_ADAGRAD == 1


@pytest.mark.parametrize("opt", [0, 1])
def test_set_optimizer_on_null_model(opt):
    assert L().fmhip_model_set_optimizer(None, opt, 1e-10, 0.1) == -1
    assert "NULL" in L().fmhip_last_error().decode()


def test_optimizer_state_io_on_null_model():
    n0 = C.c_double()
    buf = np.zeros(4)
    assert L().fmhip_model_get_optimizer_state(None, C.byref(n0), buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)) == -1
    assert L().fmhip_model_set_optimizer_state(None, 0.0, buf.ctypes.data_as(C.c_void_p), buf.ctypes.data_as(C.c_void_p)) == -1
    assert L().fmhip_model_set_optimizer_state(None, 0.0, None, None) == -1


def test_optimizer_codes():
    from sparkfm_amd import _ffi
    assert _ffi.optimizer_code("sgd") == _ffi.OPT_SGD and _ffi.optimizer_code("adagrad") == _ffi.OPT_ADAGRAD
    for bad in ("adam", "AdaGrad", "", None, 1):
        with pytest.raises(ValueError):
            _ffi.optimizer_code(bad)


@pytest.mark.parametrize("kw", [dict(optimizer="adam"), dict(optimizer="ftrl"), dict(optimizer="adagrad", adagrad_eps=0.0),
                                dict(optimizer="adagrad", adagrad_eps=-1.0), dict(optimizer="adagrad", adagrad_init=-0.5),
                                dict(optimizer="adagrad", adagrad_init=math.nan), dict(adagrad_eps=math.inf)])
def test_learners_validate_optimizer(kw):
    """HipSGD, DataParallelSGD and HipDataParallelSGD refuse an unknown optimizer or bad AdaGrad settings at construction."""
    from sparkfm_amd import HipSGD
    from sparkfm_amd.distributed import DataParallelSGD, HipDataParallelSGD
    with pytest.raises(ValueError):
        HipSGD(**kw)
    with pytest.raises(ValueError):
        DataParallelSGD(**kw)
    with pytest.raises(ValueError):
        HipDataParallelSGD(None, **kw)        # (validated before the communicator is touched)


def test_learners_default_to_sgd_with_the_usual_adagrad_settings():
    from sparkfm_amd import HipSGD
    from sparkfm_amd.distributed import DataParallelSGD
    for obj in (HipSGD(), DataParallelSGD(), HipSGD(optimizer="adagrad")):
        assert obj.adagrad_eps == 1e-10 and obj.adagrad_init == 0.1
    assert HipSGD().optimizer == "sgd" and DataParallelSGD().optimizer == "sgd"


def test_data_parallel_engine_without_the_call_refuses_adagrad():
    """DataParallelSGD sets the optimizer through its engine before every step; an engine that cannot raises ValueError (as it
    does for the loss)."""
    from sparkfm_amd.distributed import DataParallelSGD

    class Engine:                      # no set_loss, no set_optimizer
        n_batches = 1
        grad = None

        def compute(self, j):
            raise AssertionError("must not be reached")

    with pytest.raises(ValueError, match="SGD"):
        DataParallelSGD(optimizer="adagrad").step(Engine(), 0)


def test_reference_rule_matches_torch_adagrad():
    """train_ref.adagrad_rule (what every GPU test compares against) against torch.optim.Adagrad in fp64 on a small dense
    FM-like problem: three param groups (w0, w, V) each with its own weight_decay, the initial accumulator and eps of the
    library's defaults, several steps of a changing gradient."""
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(5)
    w0, w, v = rng.normal(0, 0.1, 1), rng.normal(0, 0.1, 7), rng.normal(0, 0.1, (3, 7))
    regs, eta, eps, init = (0.0, 1e-2, 3e-2), 0.07, 1e-10, 0.1
    tp = [torch.tensor(p.copy(), dtype=torch.float64, requires_grad=True) for p in (w0, w, v)]
    opt = torch.optim.Adagrad([{"params": [t], "weight_decay": r} for t, r in zip(tp, regs)], lr=eta, lr_decay=0.0,
                              initial_accumulator_value=init, eps=eps)
    ours = [p.copy() for p in (w0, w, v)]
    acc = [np.full(p.shape, init) for p in ours]
    for it in range(6):
        grads = [rng.normal(0, 1.0 / (1 + it), p.shape) for p in ours]
        grads[1][it % 7] = 0.0                        # a coordinate without a gradient still decays (weight_decay)
        for t, g in zip(tp, grads):
            t.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        for j, (g, r) in enumerate(zip(grads, regs)):
            ours[j], acc[j] = adagrad_rule(ours[j], acc[j], g + r * ours[j], eta, eps)
    for j, t in enumerate(tp):
        np.testing.assert_allclose(ours[j], t.detach().numpy(), rtol=1e-13, atol=1e-15)
        np.testing.assert_allclose(acc[j], opt.state[t]["sum"].numpy(), rtol=1e-13, atol=1e-15)


def test_reference_rule_without_decay_leaves_untouched_coordinates_alone():
    """The basis of the rows-only AdaGrad update (reg = 0): a zero g_hat moves neither the accumulator nor the value,
    whatever the accumulator holds (even 0)."""
    th, n = np.array([0.3, -1.0, 0.0]), np.array([0.0, 0.1, 5.0])
    t2, n2 = adagrad_rule(th, n, np.zeros(3), 0.5, 1e-10)
    assert np.array_equal(t2, th) and np.array_equal(n2, n)
