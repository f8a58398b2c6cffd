"""The backward arithmetic switch of the DAC baseline codec (DAC.set_grad_precision, include/escx.h escx_dac_set_grad_precision): what can be
checked without a device - the two symbols, the Python setter's names, refusals and its independence of set_precision."""
import ctypes

import pytest

import dac_grad_util as gu


def _model():
    from esc.baselines import DAC
    return DAC(**gu.config("dac_syn"))


def test_symbols_are_declared_and_exported():
    from esc import _native
    lib = _native.load()
    want = {"escx_dac_set_grad_precision": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]), "escx_dac_get_grad_precision": (ctypes.c_int, [ctypes.c_void_p])}
    for sym, (res, args) in want.items():
        assert sym in _native.SIGNATURES, sym
        assert _native.SIGNATURES[sym][0] is res and list(_native.SIGNATURES[sym][1]) == args, sym
        assert hasattr(lib, sym), sym
    # the null-handle answers need no device
    assert lib.escx_dac_get_grad_precision(None) == -1
    assert lib.escx_dac_set_grad_precision(None, 0) == _native.ESCX_ERR_INVALID_ARG


def test_default_round_trip_and_return_value():
    m = _model()
    assert m.grad_precision == "fp32"
    assert m.set_grad_precision("bf16x3") is m and m.grad_precision == "bf16x3"
    assert m.set_grad_precision("fp32") is m and m.grad_precision == "fp32"


@pytest.mark.parametrize("before", ("fp32", "bf16x3"))
def test_f16x2_is_refused_and_leaves_the_mode(before):
    m = _model().set_grad_precision(before)
    with pytest.raises(NotImplementedError):
        m.set_grad_precision("f16x2")
    assert m.grad_precision == before


@pytest.mark.parametrize("bad", ("bf16", "", None, 3))
def test_unknown_names_are_value_errors(bad):
    m = _model().set_grad_precision("bf16x3")
    with pytest.raises(ValueError, match="precision"):
        m.set_grad_precision(bad)
    assert m.grad_precision == "bf16x3"


def test_the_two_setters_do_not_move_each_other():
    m = _model()
    for fwd in ("fp32", "bf16x3"):
        for bwd in ("fp32", "bf16x3"):
            m.set_precision(fwd)
            m.set_grad_precision(bwd)
            assert (m.precision, m.grad_precision) == (fwd, bwd)
            m.set_precision("fp32" if fwd == "bf16x3" else "bf16x3")
            assert m.grad_precision == bwd
            m.set_precision(fwd)
            m.set_grad_precision("fp32" if bwd == "bf16x3" else "bf16x3")
            assert m.precision == fwd
