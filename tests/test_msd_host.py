"""Multi-scale discriminator (MSD, `Discriminator(rates=[...])`), host side: the torch restatement of tests/msd_util.py against the fixture
of the REAL reference (tests/golden/msd.npz, tools/gen_msd_golden.py), the state-dict contract of esc.models.Discriminator and its
argument errors.  No GPU needed.
"""
import json
import os

import numpy as np
import pytest
import torch

import msd_util as mu
from conftest import GOLDEN


def test_restatement_matches_the_reference_fixture():
    """Losses, gradient norms, the waveform gradient and the feature maps of configuration A (rates [1, 2, 4], one period, one window
    length, B = 3, L = 2001) against the reference Discriminator + GANLoss, with the bounds of test_oracle_discriminator_matches_reference.
    This pins the MSD's convolutions (grouping, strides, padding, weight norm, activations), their order among the sub-discriminators and
    the losses.  The resampler is the SAME code on both sides (the reference's audiotools call is not installed): it is
    not pinned by this test."""
    g, man, sd, real, fake = mu.fixture_a()
    cfg = json.loads(str(g["cfg_json"]))
    assert cfg == mu.CFG_A
    sd = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    fake = fake.clone().requires_grad_(True)
    ld = mu.gan_discriminator_loss(fake, real, sd, cfg)
    ld.mean().backward()
    np.testing.assert_allclose(ld.detach().numpy(), g["disc_loss"], rtol=1e-5)
    keys = json.loads(str(g["keys_json"]))
    gn = np.array([float(sd[k].grad.double().norm()) for k in keys])
    np.testing.assert_allclose(gn, g["disc_gnorm"], rtol=2e-4, atol=1e-9)
    for v in sd.values():
        v.grad = None
    lg, lf = mu.gan_generator_loss(fake, real, sd, cfg)
    (lg + 2.0 * lf).mean().backward()
    np.testing.assert_allclose(lg.detach().numpy(), g["gen_loss"], rtol=1e-5)
    np.testing.assert_allclose(lf.detach().numpy(), g["feat_loss"], rtol=1e-5)
    assert mu.rel(fake.grad.numpy(), g["d_fake"]) < 1e-4
    fm = mu.discriminator_forward(fake.detach().unsqueeze(1), {k: v.detach() for k, v in sd.items()}, cfg)
    shapes = json.loads(str(g["fmap_shapes_json"]))
    assert [[list(t.shape) for t in f] for f in fm] == shapes
    for r, i in zip(cfg["rates"], range(len(cfg["periods"]), len(cfg["periods"]) + len(cfg["rates"]))):
        assert [s[2] for s in shapes[i]] == {1: [2001, 501, 126, 32, 8, 8, 8], 2: [1000, 250, 63, 16, 4, 4, 4], 4: [500, 125, 32, 8, 2, 2, 2]}[r]
    for i, f in enumerate(fm):
        np.testing.assert_allclose([float(t.double().pow(2).mean().sqrt()) for t in f], g["fmap_rms"][i][: len(f)], rtol=1e-4)


def test_resampler_restatement_properties():
    """The FIR of DESIGN.md 14.1: tap counts, unit DC gain, a tone in the pass band comes through, a tone above the new Nyquist does not."""
    for rate, width in ((2, 51), (4, 102)):
        k, w = mu.resample_taps(rate)
        assert w == width and len(k) == 2 * width + rate and abs(k.sum() - 1.0) < 1e-15
        n = torch.arange(16000, dtype=torch.float64)
        const = torch.full((1, 1, 16000), 0.37, dtype=torch.float64)
        assert float((mu.resample(const, rate) - 0.37).abs().max()) < 1e-15
        lo = torch.sin(2 * np.pi * 440.0 * n / 16000.0).view(1, 1, -1)
        want = torch.sin(2 * np.pi * 440.0 * torch.arange(16000 // rate, dtype=torch.float64) * rate / 16000.0)
        y = mu.resample(lo, rate)[0, 0]
        assert y.shape[0] == 16000 // rate
        assert float((y - want)[200:-200].abs().max()) < 1e-4      # (the sinc is centred on sample n * rate: no delay; edges left out)
        hi = torch.sin(2 * np.pi * 7000.0 * n / 16000.0).view(1, 1, -1)
        assert float(mu.resample(hi, rate)[0, 0, 200:-200].abs().max()) < 2e-4


def test_state_dict_contract():
    from esc.models import Discriminator
    g, man, sd, _, _ = mu.fixture_a()
    disc = Discriminator(**mu.CFG_A)
    assert {k: list(v.shape) for k, v in disc.state_dict().items()} == man
    assert list(disc.state_dict()) == list(man)
    assert [k for k, _ in disc.named_parameters()] == json.loads(str(g["keys_json"]))
    disc.load_state_dict(sd, strict=True)
    p = "discriminators.2."                    # periods [3], rates [1, 2, 4]: the second MSD
    assert tuple(disc.state_dict()[p + "convs.4.0.weight_v"].shape) == (1024, 4, 41) and tuple(disc.state_dict()[p + "convs.4.0.weight_g"].shape) == (1024, 1, 1)
    v, gg = disc.state_dict()[p + "convs.1.0.weight_v"], disc.state_dict()[p + "convs.1.0.weight_g"]
    fresh = Discriminator(**mu.CFG_A).state_dict()
    torch.testing.assert_close(fresh[p + "convs.1.0.weight_g"].flatten(), fresh[p + "convs.1.0.weight_v"].flatten(1).norm(dim=1))      # weight_norm's init: g = ||v||
    assert float(fresh[p + "convs.1.0.weight_v"].abs().max()) <= 1.0 / np.sqrt(4 * 41)


def test_no_rates_is_the_discriminator_of_before():
    from esc.models import Discriminator
    man = json.load(open(os.path.join(GOLDEN, "disc_manifest.json")))
    disc = Discriminator(rates=[], sample_rate=16000)
    assert list(disc.state_dict()) == list(man)
    assert {k: list(v.shape) for k, v in disc.state_dict().items()} == man


def test_argument_errors():
    from esc.models import Discriminator
    with pytest.raises(NotImplementedError, match="divide"):
        Discriminator(rates=[3], periods=[2], fft_sizes=[256], sample_rate=16000)
    with pytest.raises(ValueError):
        Discriminator(rates=[1] * 9, periods=[2], fft_sizes=[256], sample_rate=16000)
    with pytest.raises(ValueError):
        Discriminator(rates=[0], periods=[2], fft_sizes=[256], sample_rate=16000)
