"""CPU-side checks of the decoder's parameter gradients (esc.baselines.DAC.set_trainable, include/escx.h escx_dac_decode_backward_params): the
library exports and binds the new entry points, the float64 restatement of tests/dac_util.py reproduces the REAL reference's parameter-gradient
fixture (tools/gen_dac_param_grad_golden.py), and the switch validates, round-trips and leaves training mode refused.  No GPU here."""
import os

import numpy as np
import pytest
import torch

import dac_grad_util as gu
import dac_param_grad_util as pu
from conftest import load_golden

NEW_SYMBOLS = ("escx_dac_decode_backward_params", "escx_dac_param_grad_workspace_floats", "escx_dac_param_grad_slices")


def test_library_exports_and_binds_the_parameter_gradient_entry_points():
    from esc import _native
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert name in _native.SIGNATURES, name
        fn = getattr(lib, name)
        restype, argtypes = _native.SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


@pytest.mark.parametrize("name", sorted(pu.FIXTURE_CASES))
def test_float64_restatement_reproduces_the_reference_parameter_gradients(name):
    g = load_golden("dac_param_grad")
    B, T = pu.FIXTURE_CASES[name]
    z, w = g[f"{name}_z"], g[f"{name}_w"]
    zi, wi = gu.inputs(name, B, T)
    assert z.dtype == w.dtype == np.float64 and np.array_equal(z, zi) and np.array_equal(w, wi), "the fixture's inputs are not the seeded ones"
    own = pu.oracle(name, z, w)
    keys = pu.decoder_keys(gu.state_dict(name))
    assert list(own) == keys and len(keys) == {"dac_syn": 63, "dac_tiny": 119}[name]
    worst, full, sampled = 0.0, 0, 0
    for k in keys:
        if pu.kind(k) in pu.SAMPLED.get(name, ()):
            idx = pu.sample_index(k, own[k].size)
            want_s, want_n = g[f"{name}_s/{k}"], float(g[f"{name}_n/{k}"])
            assert 0 < len(idx) <= pu.MAX_SAMPLES and want_s.shape == idx.shape and want_s.dtype == np.float64 and want_n > 0
            assert f"{name}_g/{k}" not in g.files
            e = max(float(np.linalg.norm(own[k].ravel()[idx] - want_s)) / float(np.linalg.norm(want_s)), abs(float(np.linalg.norm(own[k].ravel())) - want_n) / want_n)
            sampled += 1
        else:
            want = g[f"{name}_g/{k}"]
            assert want.dtype == np.float64 and want.shape == own[k].shape and np.any(want != 0), k
            e = gu.rel_l2(own[k], want)
            full += 1
        worst = max(worst, e)
        assert e <= 1e-12, (k, e)
    print(f"{name}: {full} full tensors, {sampled} sampled; float64 restatement vs reference, worst tensor {worst:.3e}")
    assert sampled == {"dac_syn": 0, "dac_tiny": 2 + 7 * 4}[name]          # dac_tiny: one weight_v per decoder convolution


def test_fixture_is_small():
    assert os.path.getsize(os.path.join(gu.GOLD, "dac_param_grad.npz")) < 400_000


def test_set_trainable_validates_round_trips_and_training_mode_still_refuses():
    from esc.baselines import DAC
    m = DAC(**gu.config("dac_syn"))                             # never touches a device
    assert m.trainable is None
    assert m.set_trainable("decoder") is m and m.trainable == "decoder"
    for part in ("encoder", "quantizer", "all"):
        with pytest.raises(NotImplementedError, match="decoder"):
            m.set_trainable(part)
        assert m.trainable == "decoder"
    for part in ("Decoder", "", 0, True, ("decoder",)):
        with pytest.raises(ValueError):
            m.set_trainable(part)
        assert m.trainable == "decoder"
    m.train()
    for p in m.parameters():
        p.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        m.decode(torch.zeros(1, m.latent_dim, 3, requires_grad=True))
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 1, 64))
    assert all(p.grad is None for p in m.parameters())
    assert m.eval().set_trainable(None) is m and m.trainable is None


def test_decoder_parameters_are_the_decoder_keys_in_state_dict_order():
    from esc.baselines import DAC
    for name in ("dac_syn", "dac_tiny"):
        m = DAC(**gu.config(name))
        want = [k for k in m.state_dict() if k.startswith("decoder.")]
        named = dict(m.named_parameters())
        got = list(m.decoder_parameters())
        assert len(got) == len(want) == {"dac_syn": 63, "dac_tiny": 119}[name]
        assert all(p is named[k] for p, k in zip(got, want))
