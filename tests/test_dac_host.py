"""The DAC baseline codec (esc.baselines.DAC) on the CPU: state_dict layout and strict loads, the torch restatement (tests/dac_util.py) against the
real reference's fixtures (tools/gen_dac_golden.py), the length arithmetic, the checkpoint loader and the argument errors."""
import json
import math

import numpy as np
import pytest
import torch

import dac_util as du
from conftest import load_golden, load_manifest
from esc import synth

NAMES = ("dac_syn", "dac_tiny", "dac_base")


def _cfg(name):
    return json.loads(str(load_golden(name)["config_json"]))


def _sd(name):
    return {k: torch.from_numpy(v) for k, v in synth.dac_state_dict(load_manifest(name)).items()}


def _x(pcm):
    return torch.from_numpy(synth.pcm_to_float(pcm))[:, None]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_layout_and_strict_load(name):
    from esc.baselines import DAC
    man = load_manifest(name)
    m = DAC(**_cfg(name))
    assert [(k, list(v.shape)) for k, v in m.state_dict().items()] == list(man.items())
    assert [k for k, _ in m.named_parameters()] == list(man)
    m.load_state_dict(_sd(name), strict=True)
    if name != "dac_syn":
        assert len(man) == 364
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in _sd(name).items() if "codebook" not in k}, strict=True)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(name):
    g = load_golden(name)
    ref = du.DacRef(_cfg(name), _sd(name))
    x = _x(g["pcm"])
    with torch.no_grad():
        zz = ref.encoder(x)
        for n in du.GOLDEN_NS:
            k = du.nkey(n)
            z, codes, lat, cm, cb, _ = ref.quantize(zz, n)
            np.testing.assert_array_equal(codes.numpy(), g[f"codes_{k}"])
            assert lat.shape[1] == g[f"codes_{k}"].shape[1] * ref.cfg["codebook_dim"]
            np.testing.assert_allclose(lat.numpy(), g["latents"][:, :lat.shape[1]], rtol=0, atol=1e-5 * np.abs(g["latents"]).max())
            np.testing.assert_allclose(float(cm), float(g[f"cm_{k}"]), rtol=1e-5)
            np.testing.assert_allclose(float(cb), float(g[f"cb_{k}"]), rtol=1e-5)
            if f"z_{k}" in g:
                assert _rel(z, g[f"z_{k}"]) < 1e-5
            if f"audio_{k}" in g:
                assert _rel(ref.decoder(z), g[f"audio_{k}"]) < 1e-5
        fz = ref.from_codes(torch.from_numpy(g["codes_nall"].astype(np.int64)))[0]
        assert _rel(fz, g["fc_z"]) < 1e-5
        fw = ref.forward(_x(g["fwd_pcm"]))
    assert fw["audio"].shape[-1] == g["fwd_pcm"].shape[-1]
    np.testing.assert_array_equal(fw["codes"].numpy(), g["fwd_codes"])
    assert _rel(fw["audio"], g["fwd_audio"]) < 1e-5


@pytest.mark.parametrize("name", NAMES)
def test_length_helpers(name):
    from esc.baselines import DAC
    g = load_golden(name)
    cfg = _cfg(name)
    m = DAC(**cfg)
    L = g["pcm"].shape[-1]
    T = g["codes_nall"].shape[-1]
    assert m.num_frames(L) == du.num_frames(cfg, L) == T
    assert m.output_samples(T) == du.output_samples(cfg, T) == int(g["decode_len"][0])
    L2 = g["fwd_pcm"].shape[-1]
    hop = int(g["hop"][0])
    assert m.hop_length == hop and L2 % hop != 0
    assert m.num_frames(math.ceil(L2 / hop) * hop) == g["fwd_codes"].shape[-1] == int(g["fwd_z_shape"][2])
    if cfg["decoder_rates"] == [8, 5, 4, 2]:
        assert m.output_samples(T) == 320 * T - 8 == 15992
        assert m.num_frames(16123) == 50 and m.num_frames(16320) == 51
    for L in list(range(1, 3 * hop, 7)) + [hop - 1, hop, hop + 1]:
        assert m.num_frames(L) == du.num_frames(cfg, L) if du.num_frames(cfg, L) > 0 else m.num_frames(L) == 0
    assert m.num_frames(hop) == 1 and m.num_frames(hop // 4) == 0


def test_argument_errors_without_a_device():
    from esc.baselines import DAC
    m = DAC(**_cfg("dac_syn"))
    x = torch.zeros(1, 1, 1600)
    with pytest.raises(NotImplementedError):
        m.encode(x)                                   # training mode (the default after construction)
    m.eval()
    with pytest.raises(RuntimeError, match="HIP device"):
        m.encode(x)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.decode(torch.zeros(1, 32, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        m(x)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.quantizer.from_codes(torch.zeros(1, 2, 4, dtype=torch.int64))
    with pytest.raises(ValueError):
        m._n_quantizers(0)
    assert m._n_quantizers(None) == 4 and m._n_quantizers(2) == 2 and m._n_quantizers(18) == 4
    with pytest.raises(AssertionError):
        m.preprocess(x, 44100)
    assert m.preprocess(torch.zeros(1, 1, 1603), 16000).shape[-1] == 1604


def test_load_of_a_save_to_folder_layout(tmp_path):
    from esc.baselines import DAC
    cfg = _cfg("dac_syn")
    sd = _sd("dac_syn")
    p = tmp_path / "dac" / "weights.pth"
    p.parent.mkdir()
    torch.save({"state_dict": sd, "metadata": {"kwargs": dict(cfg, quantizer_dropout=0.5)}}, str(p))
    m = DAC.load(str(p))
    assert m.n_codebooks == 4 and m.sample_rate == 16000 and m.quantizer_dropout == 0.5
    for k, v in m.state_dict().items():
        assert torch.equal(v, sd[k])


def test_constructor_defaults_are_the_reference():
    from esc.baselines import DAC
    m = DAC()
    assert m.latent_dim == 1024 and m.hop_length == 512 and m.n_codebooks == 9 and m.sample_rate == 44100
    assert m.quantizer.n_codebooks == 9
