"""CPU-side checks of the encoder's and the quantiser's parameter gradients (esc.baselines.DAC.set_encode_trainable, include/escx.h
escx_dac_encode_backward_params): the library exports and binds the new entry points, the float64 restatement of
tests/dac_encode_param_grad_util.py (DacRefE with the parameters as leaves) reproduces the REAL reference's fixture
(tools/gen_dac_encode_param_grad_golden.py) within 1e-12 on every stored tensor, the switch validates without a device and is independent of
set_trainable, and the parameter lists are the state_dict's.  No GPU here."""
import os

import numpy as np
import pytest
import torch

import dac_encode_grad_util as eu
import dac_encode_param_grad_util as qu
from conftest import load_golden

NEW_SYMBOLS = ("escx_dac_encode_backward_params", "escx_dac_encode_param_grad_slices")
N_KEYS = {"dac_syn": 91, "dac_tiny": 245}


def test_library_exports_and_binds_the_new_entry_points():
    from esc import _native
    lib = _native.load()
    for name in NEW_SYMBOLS:
        assert name in _native.SIGNATURES, name
        fn = getattr(lib, name)
        restype, argtypes = _native.SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name


@pytest.mark.parametrize("name", sorted(qu.FIXTURE_CASES))
def test_float64_restatement_reproduces_the_reference_parameter_gradients(name):
    g = load_golden("dac_encode_param_grad")
    B, L, n = qu.FIXTURE_CASES[name]
    x, cot = qu.inputs(name, B, L, n)
    old = load_golden("dac_encode_grad")                        # the same x and the same cotangents as the audio-gradient fixture, which stores them
    assert np.array_equal(old[f"{name}_x"], x) and old[f"{name}_x"].dtype == np.float64, "the audio is not the seeded one"
    for k in ("z", "latents", "cm"):
        assert np.array_equal(old[f"{name}_w_{k}"], np.asarray(cot[k])), f"the cotangent on {k} is not the seeded one"
    assert np.array_equal(g[f"{name}_w_cb"], np.asarray(cot["cb"])) and g[f"{name}_w_cb"].dtype == np.float64 and float(cot["cb"]) > 0
    assert np.array_equal(g[f"{name}_codes"], old[f"{name}_codes"])
    assert np.array_equal(eu.oracle_codes(name, x, n), g[f"{name}_codes"]), "the restatement chooses other codes than the reference"
    own = qu.oracle(name, x, cot, n)
    keys = qu.encode_keys(eu.state_dict(name))
    assert list(own) == keys and len(keys) == N_KEYS[name]
    worst, full, sampled, values = 0.0, 0, 0, 0
    skeys = qu.sampled_keys(name, keys)
    norms = g[f"{name}_norms"] if skeys else np.zeros(0)
    assert norms.shape == (len(skeys),) and norms.dtype == np.float64
    for k in keys:
        assert own[k] is not None, k
        if qu.kind(k) in qu.SAMPLED.get(name, ()):
            idx = qu.sample_index(k, own[k].size)
            want_s, want_n = g[f"{name}_s/{k}"], float(norms[skeys.index(k)])
            assert 0 < len(idx) <= qu.MAX_SAMPLES and len(np.unique(idx)) == len(idx) and want_s.shape == idx.shape and want_s.dtype == np.float64 and want_n > 0
            assert f"{name}_g/{k}" not in g.files
            # against the tensor's norm: a codebook's gradient is zero in every row no frame chose, so a sample set may hold zeros only
            e = max(float(np.linalg.norm(own[k].ravel()[idx] - want_s)) / want_n, abs(float(np.linalg.norm(own[k].ravel())) - want_n) / want_n)
            sampled += 1
        else:
            want = g[f"{name}_g/{k}"]
            assert want.dtype == np.float64 and want.shape == own[k].shape and np.any(want != 0), k
            assert f"{name}_s/{k}" not in g.files
            e = eu.rel_l2(own[k], want)
            full += 1
            values += want.size
        worst = max(worst, e)
        assert e <= 1e-12, (k, e)
    print(f"{name}: {full} full tensors ({values} values), {sampled} sampled; float64 restatement vs reference, worst tensor {worst:.3e}")
    if name == "dac_syn":
        assert (full, sampled, values) == (91, 0, 16368)
    else:                                                       # one weight_v per encoder convolution and projection, one codebook per stage
        cfg = eu.config(name)
        assert sampled == (2 + 7 * len(cfg["encoder_rates"])) + 3 * cfg["n_codebooks"]
    stored = {k for k in g.files if "/" in k and k.startswith(name)}
    assert {k.split("/", 1)[1] for k in stored} == set(keys), "the fixture stores gradients of other keys than the encoder's and the quantiser's"


def test_fixture_is_no_larger_than_the_largest_dac_fixture():
    assert os.path.getsize(os.path.join(eu.GOLD, "dac_encode_param_grad.npz")) <= 508_000


def test_set_encode_trainable_validates_round_trips_and_never_touches_a_device():
    from esc.baselines import DAC
    m = DAC(**eu.config("dac_syn"))
    assert m.encode_trainable is None and m.trainable is None
    for part in ("encoder", "quantizer", "both", None, "both"):
        assert m.set_encode_trainable(part) is m and m.encode_trainable == part
    for part in ("decoder", "all", "Both", "", 0, 3, True, ("both",), ["encoder"], b"both"):
        with pytest.raises(ValueError):
            m.set_encode_trainable(part)
        assert m.encode_trainable == "both"
    # independent of decode's switch, which keeps refusing what it refused and still says where its own part is
    assert m.trainable is None and m.set_trainable("decoder").encode_trainable == "both"
    for part in ("encoder", "quantizer", "all"):
        with pytest.raises(NotImplementedError, match="decoder"):
            m.set_trainable(part)
        assert m.trainable == "decoder" and m.encode_trainable == "both"
    assert m.set_encode_trainable(None).trainable == "decoder"
    assert not m._handles and not m._flat and all(p.device.type == "cpu" for p in m.parameters())
    # training mode still refuses, before anything is launched
    m.set_encode_trainable("both").train()
    for p in m.parameters():
        p.requires_grad_(True)
    with pytest.raises(NotImplementedError):
        m.encode(torch.zeros(1, 1, 64))
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 1, 64))
    assert all(p.grad is None for p in m.parameters())


def test_parameter_lists_are_the_state_dict_keys_in_order():
    from esc.baselines import DAC
    for name in ("dac_syn", "dac_tiny"):
        m = DAC(**eu.config(name))
        named = dict(m.named_parameters())
        sd = list(m.state_dict())
        enc, qnt, dec = [k for k in sd if k.startswith("encoder.")], [k for k in sd if k.startswith("quantizer.")], [k for k in sd if k.startswith("decoder.")]
        assert enc + qnt + dec == sd and len(enc) + len(qnt) == N_KEYS[name]
        assert all(p is named[k] for p, k in zip(m.encoder_parameters(), enc)) and len(list(m.encoder_parameters())) == len(enc)
        assert all(p is named[k] for p, k in zip(m.quantizer_parameters(), qnt)) and len(list(m.quantizer_parameters())) == len(qnt)
        for part, want in (("encoder", enc), ("quantizer", qnt), ("both", enc + qnt)):
            assert [k for k, _ in m.set_encode_trainable(part)._encode_named()] == want
        assert [qu.stage_of(k) for k in qnt] == [i for i in range(m.n_codebooks) for _ in range(7)] and all(qu.stage_of(k) is None for k in enc)
