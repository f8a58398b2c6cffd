"""CPU-side checks of the decoder's latent gradient (esc.baselines.DAC.decode under autograd): the library exports and binds the new entry
points, the float64 restatement of tests/dac_util.py reproduces the REAL reference's gradient fixture (tools/gen_dac_grad_golden.py), and
training mode still refuses.  No GPU here."""
import numpy as np
import pytest
import torch

import dac_grad_util as gu
from conftest import load_golden

NEW_SYMBOLS = ("escx_dac_decode_tape_floats", "escx_dac_decode_tape", "escx_dac_decode_backward", "escx_dac_test_grad_math")


def test_library_exports_and_binds_the_gradient_entry_points():
    from esc import _native
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert name in _native.SIGNATURES, name
        fn = getattr(lib, name)
        restype, argtypes = _native.SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


@pytest.mark.parametrize("name", sorted(gu.FIXTURE_CASES))
def test_float64_restatement_reproduces_the_reference_gradient(name):
    g = load_golden("dac_grad")
    B, T = gu.FIXTURE_CASES[name]
    z, w, want = g[f"{name}_z"], g[f"{name}_w"], g[f"{name}_d_z"]
    assert z.dtype == w.dtype == want.dtype == np.float64 and z.shape == want.shape == (B, gu.du.full_config(gu.config(name))["latent_dim"], T)
    zi, wi = gu.inputs(name, B, T)
    assert np.array_equal(z, zi) and np.array_equal(w, wi), "the fixture's inputs are not the seeded ones"
    assert np.array_equal(z, z.astype(np.float32).astype(np.float64)) and np.array_equal(w, w.astype(np.float32).astype(np.float64))
    err = gu.rel_l2(gu.oracle(name, z, w), want)
    print(f"{name}: float64 restatement vs reference {err:.3e}; the reference's own float32 error {float(g[f'{name}_ref_f32_err']):.3e}")
    assert err <= 1e-12
    assert 1e-8 < float(g[f"{name}_ref_f32_err"]) < 1e-5


def test_training_mode_decode_still_refuses_with_a_latent_that_requires_grad():
    from esc.baselines import DAC
    m = DAC(**gu.config("dac_syn")).train()
    z = torch.zeros(1, m.latent_dim, 3, requires_grad=True)
    with pytest.raises(NotImplementedError):
        m.decode(z)
    assert all(p.grad is None for p in m.parameters())
