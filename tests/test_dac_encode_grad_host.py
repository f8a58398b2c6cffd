"""CPU-side checks of the audio gradient through the DAC baseline's encoder and quantiser (esc.baselines.DAC.encode under autograd): the
library exports and binds the new entry points, the float64 restatement of tests/dac_encode_grad_util.py reproduces the REAL reference's
gradient fixture (tools/gen_dac_encode_grad_golden.py), and training mode still refuses.  No GPU here."""
import numpy as np
import pytest
import torch

import dac_encode_grad_util as eu
from conftest import load_golden

NEW_SYMBOLS = ("escx_dac_encode_tape_floats", "escx_dac_encode_tape", "escx_dac_encode_backward")


def test_library_exports_and_binds_the_encode_gradient_entry_points():
    from esc import _native
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert name in _native.SIGNATURES, name
        fn = getattr(lib, name)
        restype, argtypes = _native.SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


@pytest.mark.parametrize("name", sorted(eu.FIXTURE_CASES))
def test_float64_restatement_reproduces_the_reference_gradient(name):
    g = load_golden("dac_encode_grad")
    B, L, n = eu.FIXTURE_CASES[name]
    x, want, codes = g[f"{name}_x"], g[f"{name}_d_x"], g[f"{name}_codes"].astype(np.int64)
    cot = {"z": g[f"{name}_w_z"], "latents": g[f"{name}_w_latents"], "cm": float(g[f"{name}_w_cm"])}
    D, T, n, d = eu.shapes(name, B, L, n)
    assert x.dtype == want.dtype == np.float64 and x.shape == want.shape == (B, 1, L) and codes.shape == (B, n, T)
    xi, ci = eu.inputs(name, B, L, n)
    assert np.array_equal(x, xi) and all(np.array_equal(cot[k], ci[k]) for k in cot), "the fixture's inputs are not the seeded ones"
    assert all(np.array_equal(a, np.asarray(a, np.float32).astype(np.float64)) for a in (x, cot["z"], cot["latents"], cot["cm"]))
    assert np.array_equal(eu.oracle_codes(name, x, n), codes), "the restatement chooses other codes than the reference"
    err = eu.rel_l2(eu.oracle(name, x, cot, n), want)
    forced = eu.rel_l2(eu.oracle(name, x, cot, n, codes=codes), want)
    print(f"{name}: float64 restatement vs reference {err:.3e} (codes forced {forced:.3e}); the reference's own float32 error {float(g[f'{name}_ref_f32_err']):.3e}")
    assert err <= 1e-12 and forced <= 1e-12
    assert 1e-8 < float(g[f"{name}_ref_f32_err"]) < 1e-5
    # every cotangent reaches the audio, and the detaches matter: DacRef's own quantiser (no detach) has another gradient
    for k in cot:
        assert np.linalg.norm(eu.oracle(name, x, {k: cot[k]}, n)) > 1e-3, k
    plain = eu.gu.DacRefD(eu.config(name), eu.state_dict(name))
    loose = eu.grad_of(lambda xt: dict(zip(("z", "codes", "latents", "cm"), plain.encode(xt, n))), x, cot, torch.float64)
    assert eu.rel_l2(loose, want) > 1e-3


def test_per_clip_counts_of_the_restatement_are_the_single_clip_calls():
    name, (B, L, n) = "dac_syn", eu.FIXTURE_CASES["dac_syn"]
    x, cot = eu.inputs(name, B, L, n)
    counts = [1, 4, 2]
    D, T, n, d = eu.shapes(name, B, L, n)
    got = eu.oracle(name, x, {k: cot[k] for k in ("z", "latents")}, n, counts=counts)
    for b, nb in enumerate(counts):
        one = eu.oracle(name, x[b:b + 1], {"z": cot["z"][b:b + 1], "latents": cot["latents"][b:b + 1, :nb * d]}, nb)
        assert eu.rel_l2(got[b:b + 1], one) < 1e-13, b


def test_training_mode_encode_still_refuses_with_an_input_that_requires_grad():
    from esc.baselines import DAC
    m = DAC(**eu.config("dac_syn")).train()
    x = torch.zeros(1, 1, 28, requires_grad=True)
    with pytest.raises(NotImplementedError):
        m.encode(x)
    with pytest.raises(NotImplementedError):
        m.encode(x, [2])
    with pytest.raises(NotImplementedError):
        m(x)
    assert x.grad is None and all(p.grad is None for p in m.parameters())
