"""The DAC baseline's adversarial step on the MI355X: esc.baselines.GANLoss and scripts/train_dac.py --adv against tests/golden/dac_adv.npz, the sequence
recorded from the real reference classes (tools/gen_dac_adv_golden.py).  test_dac_adv_host.py asserts, on the host, the conditions these bounds rest on.

Bounds (tests/dac_adv_util.py): a stored quantity may be max(T, 4 x the reference's own float32 error on it) from the float64 value, T being what
tests/test_disc.py allows for the same kind of quantity.  Every test prints the device's measured errors before it asserts.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dac_adv_util as A
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "dac_adv.npz"))


def _disc():
    from esc.baselines import Discriminator
    disc = Discriminator(**A.YML_DISC)
    disc.load_state_dict(A.disc_state(), strict=True)
    return disc.to(DEV)


def _signals(grad=False):
    fake, real = A.signals()
    return fake.to(DEV).requires_grad_(grad), real.to(DEV)


def _check(g, name, got):
    err, bound = A.error(g, name, got), A.tol(g, name)
    print(f"[dac-adv {name}] device error {err:.2e}  bound {bound:.2e}  (reference float32 {A.reference_error(g, name):.2e})")
    assert err <= bound, name


def _np(t):
    return t.detach().cpu().numpy()


def test_loss_values(g):
    from esc.baselines import GANLoss
    from esc.modules import GANLoss as PerClip
    gan = GANLoss(_disc())
    fake, real = _signals()
    ld = gan.discriminator_loss(fake, real)
    lg, lf = gan.generator_loss(fake, real)
    assert ld.dim() == lg.dim() == lf.dim() == 0
    for name, v in (("disc_loss", ld), ("gen_before", lg), ("feat_before", lf)):
        _check(g, name, float(v.detach()))
    per = PerClip(gan.discriminator)
    pg, pf = per.generator_loss(fake, real)
    for name, v, p in (("disc", ld, per.discriminator_loss(fake, real)), ("gen", lg, pg), ("feat", lf, pf)):
        assert p.shape == (2,)
        err = A.rel(v.detach(), p.detach().mean())
        print(f"[dac-adv {name}] against the per-clip class averaged: {err:.2e}")
        assert err <= 1e-6, name
    d_fake, d_real = gan(fake, real)
    assert len(d_fake) == len(d_real) == 8 and d_fake[0][-1].shape[:2] == (2, 1)


def test_gradients(g):
    from esc.baselines import GANLoss
    disc = _disc()
    gan = GANLoss(disc)
    fake, real = _signals(grad=True)
    assert all(p.grad is None for p in disc.parameters())
    lg, lf = gan.generator_loss(fake, real)
    (A.W_GEN * lg + A.W_FEAT * lf).backward()
    assert all(p.grad is None for p in disc.parameters())              # generator_loss deposits nothing in the discriminator
    _check(g, "d_fake_before", _np(fake.grad))
    fake.grad = None
    gan.discriminator_loss(fake, real).backward()
    assert fake.grad is None
    for k, p in disc.named_parameters():
        assert p.grad is not None and bool(p.grad.any()) and bool(torch.isfinite(p.grad).all()), k
    kept = [p.grad.clone() for p in disc.parameters()]
    lg, lf = gan.generator_loss(fake, real)
    (lg + lf).backward()
    assert fake.grad is not None and all(torch.equal(p.grad, k) for p, k in zip(disc.parameters(), kept))


def test_discriminator_gradients_against_the_per_clip_class():
    """d discriminator_loss / d parameters (one forward over [fake | real], the backward per half) against
    esc.modules.GANLoss.discriminator_loss(...).mean().backward() (two passes) on a copy of the weights: relative RMS at most 1e-6 per tensor.
    A single backward over all four clips misses this bound on one tensor of 324 (`discriminators.1.conv_post.weight_g`, a single number: 1.27e-6, where the
    fake and the real half nearly cancel); esc.baselines.loss._DiscLossFn says why the backward is run per half."""
    from esc.baselines import GANLoss
    from esc.modules import GANLoss as PerClip
    disc, other = _disc(), _disc()
    fake, real = _signals()
    GANLoss(disc).discriminator_loss(fake, real).backward()
    PerClip(other).discriminator_loss(fake, real).mean().backward()
    errs = sorted(((A.rel_rms(_np(p.grad), _np(q.grad)), k) for (k, p), q in zip(disc.named_parameters(), other.parameters())), reverse=True)
    print("[dac-adv] discriminator gradients, one pass over [fake | real] against the per-clip class's two passes: " + "  ".join(f"{k} {e:.2e}" for e, k in errs[:3]))
    assert errs[0][0] <= 1e-6, errs[0]


def test_one_pass_per_loss_call():
    from esc.baselines import GANLoss
    disc = _disc()
    gan = GANLoss(disc)
    calls, inner = [], disc.forward

    def counted(x, *a, **k):
        calls.append(x.shape[0])
        return inner(x, *a, **k)

    disc.forward = counted
    fake, real = _signals(grad=True)
    gan.discriminator_loss(fake, real)
    assert calls == [4]
    del calls[:]
    gan.generator_loss(fake, real)
    assert calls == [4]
    del calls[:]
    short = fake[..., :2000]
    two = gan.discriminator_loss(short, real)
    assert calls == [2, 2] and two.dim() == 0 and bool(torch.isfinite(two))
    del calls[:]
    with pytest.raises(RuntimeError):                    # feature matching compares maps of equal size
        gan.generator_loss(short, real)
    assert calls == []


def _reference_order():
    from esc.baselines import GANLoss
    from scripts import train_dac as T
    disc = _disc()
    gan = GANLoss(disc)
    opt = torch.optim.AdamW(disc.parameters(), lr=A.LR, betas=A.BETAS)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, T.OPTIM["ExponentialLR"]["gamma"])
    fake, real = _signals(grad=True)
    out = T.discriminator_update(gan, opt, sched, fake, real)
    assert fake.grad is None
    lg, lf = gan.generator_loss(fake, real)
    (A.W_GEN * lg + A.W_FEAT * lf).backward()
    torch.cuda.synchronize()
    return {"disc_loss": float(out["adv/disc_loss"]), "grad_norm_d": float(out["other/grad_norm_d"]), "gen_loss": float(lg.detach()), "feat_loss": float(lf.detach()),
            "d_fake": _np(fake.grad)}


def test_reference_order(g):
    """The discriminator's update of scripts.train_dac, then generator_loss: the fixture's AFTER-update values."""
    got = _reference_order()
    for name, v in got.items():
        _check(g, name, v)
    for after, before in (("gen_loss", "gen_before"), ("feat_loss", "feat_before")):
        change = A.rel(got[after], g[f"{before}_f64"])
        print(f"[dac-adv {after}] {change / A.tol(g, after):.0f} tolerances from the before-update value")
        assert change > A.MIN_CHANGE * A.tol(g, after)
    again = _reference_order()
    for name, v in got.items():
        assert np.array_equal(v, again[name]), name


def _tiny_model():
    import json
    from esc import synth
    from esc.baselines import DAC
    cfg = json.loads(str(np.load(os.path.join(GOLDEN, "dac_tiny.npz"))["config_json"]))
    model = DAC(**cfg)
    man = json.load(open(os.path.join(GOLDEN, "dac_tiny_manifest.json")))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.dac_state_dict(man).items()}, strict=True)
    return model.to(DEV).eval()


def test_whole_step_on_dac_tiny():
    from esc.baselines import GANLoss
    from scripts import train_dac as T
    model = _tiny_model()
    model.quantizer_dropout = 0.5
    model.set_trainable("decoder").set_encode_trainable("both")
    losses = T.make_losses(T.YML_LOSSES, model.sample_rate)
    disc = _disc()
    gan = GANLoss(disc)
    opt = torch.optim.AdamW(disc.parameters(), lr=A.LR, betas=A.BETAS)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, T.OPTIM["ExponentialLR"]["gamma"])
    before = {k: v.clone() for k, v in disc.state_dict().items()}
    signal = (0.1 * torch.randn(2, 1, 2560, generator=torch.Generator().manual_seed(3))).to(DEV)
    nq = model.sample_n_quantizers(2, torch.Generator().manual_seed(3))
    lam = dict(T.LAMBDAS)
    hook = {}
    out = T.train_step_losses(model, losses, signal, nq, lam, audio_hook=lambda a: hook.setdefault("audio", a), adv=(gan, opt, sched))
    d_grads = [p.grad.clone() for p in disc.parameters()]
    out["loss"].backward()
    torch.cuda.synchronize()
    audio = hook["audio"]
    signal = signal[..., :audio.shape[-1]]
    assert audio.shape == (2, 1, A.L) and min(nq) < max(nq)
    assert {"adv/disc_loss", "adv/gen_loss", "adv/feat_loss", "other/grad_norm_d"} <= set(out)
    # the reported generator terms are those of the UPDATED discriminator
    lg, lf = gan.generator_loss(audio.detach(), signal)
    lg, lf = lg.detach(), lf.detach()
    assert float(lg) == float(out["adv/gen_loss"]) and float(lf) == float(out["adv/feat_loss"])
    for k, v in disc.state_dict().items():
        assert not torch.equal(v, before[k]), k
    fresh = GANLoss(_disc())
    fg, ff = fresh.generator_loss(audio.detach(), signal)
    assert float(fg) != float(lg) and float(ff) != float(lf)
    terms = [k for k in lam if k in out]
    assert set(terms) == {"mel/loss", "adv/gen_loss", "adv/feat_loss", "vq/commitment_loss", "vq/codebook_loss"}
    total = sum(lam[k] * float(out[k]) for k in terms)
    print(f"[dac-adv step] " + "  ".join(f"{k} {float(v):.6g}" for k, v in sorted(out.items())))
    assert A.rel(out["loss"].detach(), total) <= 1e-6
    for key, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), key
    # d loss / d audio = the lambda-weighted sum of the unit gradients, the two adversarial ones included
    units = 0
    for k in ("mel/loss", "adv/gen_loss", "adv/feat_loss"):
        a = audio.detach().clone().requires_grad_(True)
        (losses["mel"](a, signal) if k == "mel/loss" else gan.generator_loss(a, signal)[k == "adv/feat_loss"]).backward()
        assert bool(a.grad.any()), k
        units = units + lam[k] * a.grad
    err = A.rel_rms(_np(audio.grad), _np(units))
    print(f"[dac-adv step] d loss / d audio against the weighted unit gradients: {err:.2e}")
    assert err <= 1e-6
    # the discriminator's gradients are those of the discriminator loss alone (the clip scales them when their norm exceeds 10)
    assert all(torch.equal(p.grad, k) for p, k in zip(disc.parameters(), d_grads))
    alone = _disc()
    GANLoss(alone).discriminator_loss(audio.detach(), signal).backward()
    norm = float(out["other/grad_norm_d"])
    scale = min(1.0, A.CLIP_D / (norm + 1e-6))
    worst = max(A.rel_rms(_np(p.grad), _np(q.grad) * scale) for p, q in zip(disc.parameters(), alone.parameters()))
    print(f"[dac-adv step] grad_norm_d {norm:.4f}; discriminator gradients against the discriminator loss alone: worst tensor {worst:.2e}")
    assert worst <= 1e-6


def test_script_adv_and_resume(tmp_path):
    from esc.baselines import DAC, Discriminator
    from scripts import train_dac as T
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "efficient-speech-codec_amd"))
    cmd = [sys.executable, "-m", "scripts.train_dac", "--adv", "--synthetic", "dac_tiny", "--batch_size", "2", "--save_path", str(tmp_path)]
    r = subprocess.run(cmd + ["--steps", "2"], cwd=os.path.join(ROOT, "efficient-speech-codec_amd"), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    for folder in ("dac", "discriminator"):
        for name in ("weights.pth", "optimizer.pth", "scheduler.pth"):
            assert (tmp_path / "latest" / folder / name).exists(), (folder, name)
    path = tmp_path / "latest" / "dac" / "weights.pth"
    model = DAC.load(str(path))
    ck = torch.load(str(path), map_location="cpu", weights_only=False)
    assert all(torch.equal(model.state_dict()[k], v) for k, v in ck["state_dict"].items())
    ck = torch.load(str(tmp_path / "latest" / "discriminator" / "weights.pth"), map_location="cpu", weights_only=False)
    assert ck["metadata"]["kwargs"] == A.YML_DISC
    disc = Discriminator(**ck["metadata"]["kwargs"])
    disc.load_state_dict(ck["state_dict"], strict=True)
    first = A.disc_state()
    assert all(torch.equal(disc.state_dict()[k], v) for k, v in ck["state_dict"].items()) and set(ck["state_dict"]) == set(first)
    step2 = [ln for ln in r.stdout.splitlines() if ln.startswith("step 2 ") and "adv/" in ln]
    assert len(step2) == 1, r.stdout
    for key in ("adv/disc_loss", "adv/gen_loss", "adv/feat_loss", "other/grad_norm_d"):
        assert f" {key} " in step2[0], key
    gamma, lr = T.OPTIM["ExponentialLR"]["gamma"], T.OPTIM["AdamW"]["lr"]
    assert f"other/learning_rate {lr * gamma ** 2:.6g}" in step2[0]
    r = subprocess.run(cmd + ["--steps", "3", "--resume", str(tmp_path / "latest")], cwd=os.path.join(ROOT, "efficient-speech-codec_amd"), env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    steps = [ln for ln in r.stdout.splitlines() if ln.startswith("step ") and "adv/" in ln]
    assert len(steps) == 1 and steps[0].startswith("step 3 "), r.stdout
    assert f"other/learning_rate {lr * gamma ** 3:.6g}" in steps[0] and f"{lr * gamma ** 3:.6g}" != f"{lr * gamma:.6g}"
    sched = torch.load(str(tmp_path / "latest" / "discriminator" / "scheduler.pth"), map_location="cpu", weights_only=False)
    assert sched["last_epoch"] == 3
