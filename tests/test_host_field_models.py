"""The C surface the five field models that step through the FwFM share (sparkfm_amd/csrc/fmhip_field_model.h), one table over FwFM,
FmFM, DeepFM, DCN and AutoInt, no GPU: a NULL model handle, destroy(NULL), create's out and the refusals every create opens with.  The
expected codes and texts are the ones each model's unit carried before the handles shared a core."""
import ctypes as C

import pytest

# (the model's name in messages, its macros' and functions' infix, the setter of its own array's switch, arrays of its own in
#  set/get_params, outputs of model_info behind padded_factors, create's own arguments between num_factor and stream)
MODELS = [("FwFM", "FWFM", "fwfm", "set_field_weights", 1, 0, lambda: ()),
          ("FmFM", "FMFM", "fmfm", "set_field_matrices", 1, 0, lambda: ()),
          ("DeepFM", "DEEPFM", "deepfm", "set_deep", 3, 2, lambda: (1, (C.c_int32 * 1)(16))),
          ("DCN", "DCN", "dcn", "set_cross", 4, 2, lambda: (1, 16)),
          ("AutoInt", "AUTOINT", "autoint", "set_attention", 2, 3, lambda: (1, 1, 16))]


@pytest.mark.parametrize("name,macro,lower,setter,own,info_tail,create_own", MODELS, ids=[m[0] for m in MODELS])
def test_c_calls_refuse_without_a_device(name, macro, lower, setter, own, info_tail, create_own):
    from sparkfm_amd import _ffi
    L = _ffi.load()
    err = L.fmhip_last_error
    f = lambda what: getattr(L, "fmhip_%s_%s" % (lower, what))
    nulls = [None] * own
    for call in (lambda: f("model_info")(None, None, None, None, None, *[None] * info_tail), lambda: f("model_set_params")(None, 0.0, None, None, *nulls),
                 lambda: f("model_get_params")(None, None, None, None, *nulls), lambda: f("model_set_rule")(None, 0, 0, 1e-10, 1.0),
                 lambda: f("model_set_linear")(None, 1), lambda: f("model_" + setter)(None, 1),
                 lambda: f("model_get_accumulators")(None, None, None, None, *nulls), lambda: f("model_set_accumulators")(None, 0.0, None, None, *nulls),
                 lambda: f("predict")(None, None, None), lambda: f("step")(None, None, 0, 0.1, 0.0, 0.0, 0.0, 0.0, None),
                 lambda: f("epoch")(None, None, 0.1, 0.0, 0.0, 0.0, 0.0, None, None)):
        assert call() == -1 and err() == b"the %s model handle is NULL" % name.encode()
    assert f("model_destroy")(None) == 0
    assert f("model_create")(0, 10, 2, 4, *create_own(), None, None) == -1 and err() == b"out is NULL"
    h = C.c_void_p()
    for dims, code, msg in (((-1, 2, 4), -1, "num_attribute = -1: a model has at least feature 0"),
                            ((10, 0, 4), -1, "num_fields = 0: a model has at least one field"),
                            ((10, 65, 4), -5, "num_fields = 65 is above FMHIP_%s_MAX_FIELDS = 64" % macro),
                            ((10, 2, 0), -1, "num_factor = 0: a model has at least one factor"),
                            ((-1, 0, 0), -1, "num_attribute = -1: a model has at least feature 0"),          # the first in this order wins
                            ((10, 65, 0), -5, "num_fields = 65 is above FMHIP_%s_MAX_FIELDS = 64" % macro)):
        h.value = 1
        assert f("model_create")(0, *dims, *create_own(), None, C.byref(h)) == code and err() == msg.encode(), dims
        assert h.value is None          # (*out is cleared before the first refusal)
