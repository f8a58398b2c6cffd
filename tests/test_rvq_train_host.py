"""rvq+swinT training step, CPU side (`not gpu`): the differentiable restatement of tests/rvq_train_util.py is pinned to the REAL reference's
training step (tests/golden/rvq_train.npz, tools/gen_rvq_train_golden.py), the two new C-ABI entry points exist in header, binding and library,
and the Python surface refuses what it must."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
import rvq_train_util as U


@pytest.mark.parametrize("name", ["rvq_tiny", "rvq_base"])
def test_restatement_training_step_matches_reference(name):
    """Losses 1e-5 relative, codes of all num_rvqs stages equal, every gradient norm and the stored full gradients 2e-5 (the level of
    test_oracle_training_step_matches_reference); exact zeros where the reference has zeros (masked stages, frozen codebooks)."""
    g = load_golden("rvq_train")
    keys = json.loads(str(g[f"{name}_keys"]))
    w = json.loads(str(g["weights_json"]))
    x = U.fixture_clips(g, name)
    cfg = U.cfg_of(name)
    for S, freeze in json.loads(str(g["cases_json"]))[name]:
        tag = f"{name}_s{S}_f{int(freeze)}"
        out, ls, grads = U.oracle_step(name, S, freeze, x, weights=w)
        assert tuple(out["codes"].shape) == (x.shape[0], cfg["num_rvqs"], cfg["group_size"], g[f"{tag}_codes"].shape[-1])
        losses = {"cm": out["cm_loss"].detach().numpy(), "cb": out["cb_loss"].detach().numpy(), "mel": ls["mel_loss"].detach().numpy(),
                  "stft": ls["stft_loss"].detach().numpy(), "loss": ls["loss"].detach().numpy()}
        U.check_against_fixture(g, tag, keys, losses, out["codes"].numpy(), {k: v.numpy() for k, v in grads.items()}, 2e-5)
        np.testing.assert_allclose(out["margins"].numpy(), g[f"{tag}_margins"], rtol=0, atol=2e-6)
        assert float(g[f"{tag}_margins"].min()) >= U.MIN_MARGIN          # the condition every GPU comparison of codes rests on


def test_fixture_covers_every_parameter_and_the_stated_zeros():
    from esc.models import make_model
    g = load_golden("rvq_train")
    for name in ("rvq_tiny", "rvq_base"):
        keys = json.loads(str(g[f"{name}_keys"]))
        model = make_model(U.cfg_of(name), "rvq+swinT")
        assert set(keys) == {k for k, _ in model.named_parameters()}
        R = U.cfg_of(name)["num_rvqs"]
        for S, freeze in json.loads(str(g["cases_json"]))[name]:
            tag = f"{name}_s{S}_f{int(freeze)}"
            gn = dict(zip(keys, g[f"{tag}_gnorm"]))
            for k in keys:
                m = re.fullmatch(r"quantizers\.vqs\.\d+\.vqs\.(\d+)\.embedding\.weight", k)
                if m:
                    dead = freeze or int(m.group(1)) >= S
                    assert (gn[k] == 0.0) == dead, (tag, k, gn[k])
            assert R > 0 and any(f.startswith(f"{tag}_g::") and not g[f].any() for f in g.files) == (freeze or S < R)


def test_stage_arithmetic_is_the_reference_order_not_the_plain_sum():
    """The three straight-through operations in fp32, in the stated order, carry no gradient along the residual chain and reproduce what autograd
    gives: d z_e = g + 2 / (T d G) d_cm (z_e - q_0); codebook rows get 2 / (T d G) d_cb (q_i - r_i) for the live stages, zeros past them."""
    cfg = U.cfg_of("rvq_tiny")
    sd = {k: (v.double().clone().requires_grad_(True) if v.is_floating_point() and not k.endswith(".window") else v) for k, v in U.synth_state("rvq_tiny").items()}
    orc = U.RvqTrainOracle(cfg, sd)
    gen = torch.Generator().manual_seed(3)
    B, T, G, d, R, S = 2, 5, cfg["group_size"], cfg["codebook_dim"], cfg["num_rvqs"], 2
    z = torch.randn(B, T, G, d, generator=gen, dtype=torch.float64).requires_grad_(True)
    gz = torch.randn(B, T, G, d, generator=gen, dtype=torch.float64)
    wcm, wcb = torch.randn(B, generator=gen, dtype=torch.float64), torch.randn(B, generator=gen, dtype=torch.float64)
    zq, codes, _, cm, cb = orc.quantize_train(z, S, False)
    ((zq * gz).sum() + (cm * wcm).sum() + (cb * wcb).sum()).backward()
    s = 2.0 / (T * d * G)
    for m in range(G):
        r = z.detach()[:, :, m]
        for i in range(R):
            q = orc.cb(m, i).detach()[codes[:, i, m]]
            if i == 0:
                ana = gz[:, :, m] + s * wcm[:, None, None] * (r - q)
                assert float((z.grad[:, :, m] - ana).abs().max()) < 1e-14
            want = torch.zeros_like(orc.cb(m, i))
            if i < S:
                want.index_add_(0, codes[:, i, m].reshape(-1), (s * wcb[:, None, None] * (q - r)).reshape(-1, d))
            got = orc.cb(m, i).grad
            assert got is not None and float((got - want).abs().max()) < 1e-14
            if i >= S:
                assert not got.any()
            r = r - (r + (q - r))


def test_new_entry_points_in_header_binding_and_library():
    """Fails on a library without the rvq training step: the two symbols are declared, typed and exported, and refuse a null handle."""
    from esc import _native
    lib = _native.load()
    header = open(os.path.join(ROOT, "include", "escx.h")).read()
    for name, nargs in (("escx_rvq_train_forward", 15), ("escx_rvq_train_backward", 9)):
        assert re.search(rf"\bint {name}\s*\(", header), name
        assert name in _native.SIGNATURES and len(_native.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name)
    assert lib.escx_rvq_train_forward(None, None, None, None, 1, 1280, 1, 0, None, None, None, None, None, None, None) == _native.ESCX_ERR_INVALID_ARG
    assert lib.escx_rvq_train_backward(None, None, None, None, None, None, None, None, None) == _native.ESCX_ERR_INVALID_ARG
    assert lib.escx_train_tape_bytes(None) == 0 and lib.escx_train_tape_generation(None) == 0


def test_python_refusals():
    from esc import RVQCodecs
    m = RVQCodecs(**U.cfg_of("rvq_tiny")).train()
    x = torch.zeros(2, 1260)
    with pytest.raises(NotImplementedError, match="RVQCodecs training is not implemented for CPU tensors"):
        m(x, None, 4)
    with pytest.raises(NotImplementedError, match="RVQCodecs training is not implemented for CPU tensors"):
        m(x, torch.zeros(2, 48, 64, 2), 4)
    with pytest.raises(NotImplementedError, match="RVQCodecs training is not implemented for CPU tensors"):
        m(x, None, 4, freeze_codebook=True)                    # accepted in training mode: the refusal is the device's, not the option's
    with pytest.raises(ValueError, match="per-clip"):
        m(x, None, [1, 2])
    with pytest.raises(ValueError):
        m(x, None, 0)
    m.eval()
    with pytest.raises(NotImplementedError, match="freeze_codebook"):
        m(x, None, 4, freeze_codebook=True)
    assert m._code_streams == 4 and m.max_streams == 3          # the code-slot hook of the shared training step: num_rvqs, not max_streams
