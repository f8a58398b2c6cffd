"""CPU-side checks of the weight gradients' precision switch (esc.baselines.DAC.set_param_grad_precision, include/escx.h
escx_dac_set_param_grad_precision): the default, the round trip, the refusals, the independence of the other two precision switches, copies
and pickles, the refusals the switch does not lift, and the library's exports.  No GPU here."""
import copy
import pickle

import pytest
import torch

import dac_grad_util as gu

NEW_SYMBOLS = ("escx_dac_set_param_grad_precision", "escx_dac_get_param_grad_precision")


def _model():
    from esc.baselines import DAC
    return DAC(**gu.config("dac_syn"))                          # never touches a device


def test_library_exports_and_binds_the_switch():
    from esc import _native
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert name in _native.SIGNATURES, name
        fn = getattr(lib, name)
        restype, argtypes = _native.SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


def test_null_handle_is_refused_by_the_library():
    from esc import _native
    lib = _native.load()
    assert lib.escx_dac_set_param_grad_precision(None, _native.PRECISIONS["bf16x3"]) == -1
    assert lib.escx_dac_get_param_grad_precision(None) == -1


def test_default_round_trip_and_refusals():
    m = _model()
    assert m.param_grad_precision == "fp32"
    assert m.set_param_grad_precision("bf16x3") is m and m.param_grad_precision == "bf16x3"
    with pytest.raises(NotImplementedError, match="f16x2"):
        m.set_param_grad_precision("f16x2")
    assert m.param_grad_precision == "bf16x3"
    for bad in ("nope", "", 3, None):
        with pytest.raises(ValueError):
            m.set_param_grad_precision(bad)
        assert m.param_grad_precision == "bf16x3", "a refused value changed the mode"
    assert m.set_param_grad_precision("fp32") is m and m.param_grad_precision == "fp32"


def test_independent_of_the_other_two_switches():
    m = _model()
    m.set_precision("bf16x3").set_grad_precision("fp32").set_param_grad_precision("bf16x3")
    assert (m.precision, m.grad_precision, m.param_grad_precision) == ("bf16x3", "fp32", "bf16x3")
    m.set_precision("fp32").set_grad_precision("bf16x3")
    assert (m.precision, m.grad_precision, m.param_grad_precision) == ("fp32", "bf16x3", "bf16x3")
    m.set_param_grad_precision("fp32")
    assert (m.precision, m.grad_precision, m.param_grad_precision) == ("fp32", "bf16x3", "fp32")


def test_survives_deepcopy_and_pickle():
    m = _model().set_grad_precision("bf16x3").set_param_grad_precision("bf16x3")
    for twin in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert twin.param_grad_precision == "bf16x3" and twin.grad_precision == "bf16x3" and twin.precision == "fp32"
        assert twin._handles == {} and twin._flat == {}
        twin.set_param_grad_precision("fp32")
        assert m.param_grad_precision == "bf16x3"


def test_the_switch_lifts_no_refusal():
    m = _model().set_trainable("decoder").set_param_grad_precision("bf16x3")
    for part in ("encoder", "quantizer", "all"):
        with pytest.raises(NotImplementedError, match="decoder"):
            m.set_trainable(part)
    assert m.trainable == "decoder" and m.param_grad_precision == "bf16x3"
    m.train()
    for p in m.parameters():
        p.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        m.decode(torch.zeros(1, m.latent_dim, 3, requires_grad=True))
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 1, 64))
    assert all(p.grad is None for p in m.parameters())
    assert m.eval().param_grad_precision == "bf16x3"
