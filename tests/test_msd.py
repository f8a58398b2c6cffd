"""Multi-scale discriminator (MSD, `Discriminator(rates=[...])`) on the GPU: the HIP resampler, the grouped 41-tap convolutions
(csrc/disc_msd_kernels.h) and the dense MSD layers, against the fp64 restatement of tests/msd_util.py and the fixture of the real
reference (tests/golden/msd.npz).  Configuration A: rates [1, 2, 4], periods [3], fft_sizes [256], B = 3, L = 2001.
"""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import msd_util as mu
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu


def _disc(cfg, sd=None, precision=None):
    from esc.models import Discriminator
    disc = Discriminator(**cfg)
    if sd is None:
        sd = mu.synth_state({k: list(v.shape) for k, v in disc.state_dict().items()})
    disc.load_state_dict(sd, strict=True)
    if precision:
        disc.set_conv_precision(precision)
    return disc.cuda(), sd


@functools.lru_cache(maxsize=None)
def _ref_maps(which):
    """fp64 and fp32 restatement feature maps of the fake clips: configuration A, or the MSD-only discriminator on one 173-sample clip."""
    if which == "A":
        g, man, sd, real, fake = mu.fixture_a()
        cfg, x = mu.CFG_A, fake
    else:
        from esc.models import Discriminator
        cfg = dict(rates=[1, 2, 4], periods=[], fft_sizes=[], sample_rate=16000)
        sd = mu.synth_state({k: list(v.shape) for k, v in Discriminator(**cfg).state_dict().items()})
        x = mu.clips("msd-short", 1, 173)[1]
    cfg = {**cfg, "bands": cfg.get("bands", [[0.0, 1.0]])}
    f64 = mu.discriminator_forward(x.double().unsqueeze(1), {k: v.double() for k, v in sd.items()}, cfg)
    f32 = mu.discriminator_forward(x.unsqueeze(1), sd, cfg)
    return cfg, sd, x, f64, f32


@pytest.mark.parametrize("precision", ["fp32", "split"])
@pytest.mark.parametrize("which", ["A", "short"])
def test_feature_maps(which, precision):
    """Every feature map within max(2e-5, 3 x the fp32 restatement's own distance from fp64) of the fp64 restatement (rel rms; 2e-5 is
    the bound of test_disc.py).  "short": MSD only, one clip of 173 samples - the extents fall to 43 -> 11 -> 3 -> 1 at rate 4, shorter
    than the 41 taps and than the resampler's padding."""
    cfg, sd, x, f64, f32 = _ref_maps(which)
    disc, _ = _disc({k: v for k, v in cfg.items() if which == "A" or k != "bands"}, sd, precision)
    with torch.no_grad():
        fm = disc(x.cuda().unsqueeze(1))
    assert [[list(t.shape) for t in f] for f in fm] == [[list(t.shape) for t in f] for f in f64]
    if which == "A":
        assert [[list(t.shape) for t in f] for f in fm] == json.loads(str(mu.fixture_a()[0]["fmap_shapes_json"]))
    worst = 0.0
    for i, (a, b, c) in enumerate(zip(fm, f64, f32)):
        for j, (got, r64, r32) in enumerate(zip(a, b, c)):
            err, floor = mu.rel(got.cpu().numpy(), r64.numpy()), mu.rel(r32.numpy(), r64.numpy())
            bound = max(2e-5, 3.0 * floor)
            worst = max(worst, err / bound)
            assert err <= bound, f"sub-discriminator {i} map {j}: rel rms {err:.3e} (fp32 restatement {floor:.3e})"
    print(f"[msd fmaps {which} {precision}] worst error / bound {worst:.3f}")


def test_losses_and_gradients():
    """GANLoss on configuration A: losses against the reference fixture, every parameter gradient against the fp64 restatement (bound and
    floor as in test_disc.py test_gan_losses_and_gradients), gradient norms and the waveform gradient against the fixture."""
    from esc.modules import GANLoss
    g, man, sd, real, fake = mu.fixture_a()
    cfg = mu.CFG_A
    disc, _ = _disc(cfg, sd)
    gan = GANLoss(disc)
    keys = json.loads(str(g["keys_json"]))
    assert keys == [k for k, _ in disc.named_parameters()]
    ld = gan.discriminator_loss(fake.cuda(), real.cuda())
    ld.mean().backward()
    np.testing.assert_allclose(ld.detach().cpu().numpy(), g["disc_loss"], rtol=1e-5)
    osd = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    mu.gan_discriminator_loss(fake.double(), real.double(), osd, cfg).mean().backward()
    o32 = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    mu.gan_discriminator_loss(fake, real, o32, cfg).mean().backward()
    params = dict(disc.named_parameters())
    scale = float(np.sqrt(sum(float((v.grad ** 2).sum()) for v in osd.values())))
    worst = (0.0, "")
    for k, rn in zip(keys, g["disc_gnorm"]):
        ref = osd[k].grad.numpy()
        got = params[k].grad.cpu().numpy()
        den = max(np.sqrt((ref ** 2).mean()), 1e-6 * scale / np.sqrt(ref.size))
        err = float(np.sqrt(((np.asarray(got, np.float64) - ref) ** 2).mean()) / den)
        floor = float(np.sqrt(((o32[k].grad.double().numpy() - ref) ** 2).mean()) / den)
        worst = max(worst, (err / max(5e-4, 3.0 * floor), k))
        assert err < max(5e-4, 3.0 * floor), f"gradient of {k}: rel rms {err:.3e} vs the fp64 restatement (fp32 restatement: {floor:.3e})"
        assert abs(float(np.linalg.norm(got.astype(np.float64))) - rn) <= 3e-3 * max(rn, 1e-6 * scale), k
    print(f"[msd disc step] worst gradient error / bound {worst[0]:.3f} ({worst[1]})")
    for p in disc.parameters():
        p.grad = None
    fg = fake.cuda().requires_grad_(True)
    lg, lf = gan.generator_loss(fg, real.cuda())
    (lg + 2.0 * lf).mean().backward()
    np.testing.assert_allclose(lg.detach().cpu().numpy(), g["gen_loss"], rtol=1e-5)
    np.testing.assert_allclose(lf.detach().cpu().numpy(), g["feat_loss"], rtol=1e-5)
    err = mu.rel(fg.grad.cpu().numpy(), g["d_fake"])
    print(f"[msd gen step] d loss / d fake waveform rel rms {err:.2e}")
    assert err < 5e-4


def test_determinism_and_batch_independence():
    from esc.modules import GANLoss
    g, man, sd, real, fake = mu.fixture_a()
    disc, _ = _disc(mu.CFG_A, sd)
    gan = GANLoss(disc)

    def backward():
        for p in disc.parameters():
            p.grad = None
        fg = fake.cuda().requires_grad_(True)
        gan.discriminator_loss(fake.cuda(), real.cuda()).mean().backward()
        lg, lf = gan.generator_loss(fg, real.cuda())
        grads = {k: p.grad.clone() for k, p in disc.named_parameters()}
        for p in disc.parameters():
            p.grad = None
        (lg + 2.0 * lf).mean().backward()
        return grads, fg.grad.clone(), lg.detach().clone(), lf.detach().clone()
    g1, w1, lg1, lf1 = backward()
    g2, w2, _, _ = backward()
    assert all(torch.equal(g1[k], g2[k]) for k in g1), [k for k in g1 if not torch.equal(g1[k], g2[k])]
    assert torch.equal(w1, w2)
    with torch.no_grad():
        fm3 = disc(fake.cuda().unsqueeze(1))
        fm1 = disc(fake[1:2].cuda().unsqueeze(1))
    for a, b in zip(fm3, fm1):
        for x, y in zip(a, b):
            assert torch.equal(x[1:2], y)
    # one pass over [fake | real] (GANLoss.adversarial_forward) = the two-pass losses, bit for bit
    fg = fake.cuda().requires_grad_(True)
    d_fake, d_real = gan.adversarial_forward(fg, real.cuda())
    lg2, lf2 = gan.generator_loss_from(d_fake, d_real)
    (lg2 + 2.0 * lf2).mean().backward()
    assert torch.equal(lg2, lg1) and torch.equal(lf2, lf1) and torch.equal(fg.grad, w1)


def test_training_smoke():
    """Two AdvStepper steps (scripts/train.py) of the tiny generator with an MSD in the discriminator."""
    from conftest import synth_state
    sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
    from esc import synth
    from esc.models import Discriminator, make_model
    from scripts.train import AdvStepper
    cfg = json.loads(str(load_golden("tiny")["config_json"]))
    model = make_model(cfg); model.load_state_dict(synth_state("tiny")); model = model.cuda()
    disc = Discriminator(sample_rate=16000, rates=[2], periods=[3], fft_sizes=[256]).cuda()
    L = 5020
    x = torch.from_numpy(synth.pcm_to_float(np.stack([synth.voiced_clip_int16(f"msd-adv-{i}", L) for i in range(2)]))).cuda()
    st = AdvStepper(model, disc, lr=5e-4, dropout_rate=0.0, pretraining_steps=0)
    d0 = {k: v.detach().clone() for k, v in disc.state_dict().items()}
    logs = [st.step(x, n) for n in range(2)]
    assert all("disc_loss" in l for l in logs)
    assert all(np.isfinite(float(v)) for l in logs for v in l.values() if torch.is_tensor(v))
    msd = [k for k in d0 if k.startswith("discriminators.1.")]
    assert len(msd) == 21
    same = [k for k in msd if torch.equal(disc.state_dict()[k], d0[k])]
    assert not same, same
    assert len(st.opt_d.state_dict()["state"]) == len(list(disc.parameters()))
