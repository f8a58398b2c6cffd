"""Shared by test_dac_adv_host.py, test_dac_adv.py and tools/gen_dac_adv_golden.py: the inputs of tests/golden/dac_adv.npz, the sequence it records restated
on the oracle (oracle/esc_oracle.py gan_discriminator_loss / gan_generator_loss, batch means) and the bounds the GPU tests apply.

The sequence (train_customize.py:283-302 on fixed signals): generator losses with the untouched discriminator ("before"), the discriminator loss, its
backward and clip_grad_norm_(10), one AdamW(lr 1e-4, betas (0.8, 0.99)) step, then the generator losses again and the gradient of 1.0 * gen + 2.0 * feat
with respect to `fake`.  The fixture holds it twice from the real reference classes, in float64 and in float32.

Bounds.  For a stored quantity s the device may be max(T, 4 * |s32 - s64| / |s64|) from the float64 value: T is what tests/test_disc.py allows for the same
kind of quantity (loss values rtol 1e-5, gradient norms rtol 2e-4, d_fake 1e-4 relative RMS), |s32 - s64| is the reference's own float32 error on this input
(the fixture's two runs), and the factor 4 covers a device summation order that differs from ATen's.
"""
import json
import math
import os

import numpy as np
import torch

from esc import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
YML_DISC = dict(sample_rate=16000, rates=[], periods=[2, 3, 5, 7, 11], fft_sizes=[2048, 1024, 512],
                bands=[[0.0, 0.1], [0.1, 0.25], [0.25, 0.5], [0.5, 0.75], [0.75, 1.0]])
L = 2552                    # what DAC-Tiny returns for the trainer's 2560-sample clips
LR, BETAS, CLIP_D = 1e-4, (0.8, 0.99), 10.0
W_GEN, W_FEAT = 1.0, 2.0
SCALARS = ("disc_loss", "grad_norm_d", "gen_before", "feat_before", "gen_loss", "feat_loss")
VECTORS = ("d_fake_before", "d_fake")
LOSS_RTOL, GNORM_RTOL, DFAKE_TOL = 1e-5, 2e-4, 1e-4
T = {"disc_loss": LOSS_RTOL, "gen_before": LOSS_RTOL, "feat_before": LOSS_RTOL, "gen_loss": LOSS_RTOL, "feat_loss": LOSS_RTOL, "grad_norm_d": GNORM_RTOL,
     "d_fake": DFAKE_TOL, "d_fake_before": DFAKE_TOL}
RESTATEMENT_RTOL = 1e-9     # oracle against reference in float64: the same ATen operators, the means grouped per clip instead of per map
MIN_CHANGE = 100            # an after-update loss is at least this many tolerances from its before-update value


def disc_state():
    """The rule of tests/test_disc.py::disc_state (oracle/gen_disc_golden.py synth_disc_state) over tests/golden/disc_manifest.json."""
    man = json.load(open(os.path.join(GOLDEN, "disc_manifest.json")))
    out = {}
    for k, shp in man.items():
        u = synth.hashed_uniform(k, int(np.prod(shp))).reshape(shp)
        if k.endswith("weight_v"):
            out[k] = (u / math.sqrt(int(np.prod(shp[1:])))).astype(np.float32)
        elif k.endswith("bias"):
            out[k] = (0.05 * u).astype(np.float32)
    for k, shp in man.items():
        if k.endswith("weight_g"):
            v = out[k[:-1] + "v"]
            nrm = np.sqrt((v.reshape(shp[0], -1).astype(np.float64) ** 2).sum(1)).reshape(shp)
            out[k] = (nrm * (1.0 + 0.5 * synth.hashed_uniform(k, int(np.prod(shp))).reshape(shp))).astype(np.float32)
    return {k: torch.from_numpy(out[k]) for k in man}


def signals():
    """(fake, real), float32 (2, 1, L)."""
    real = torch.from_numpy(synth.pcm_to_float(np.stack([synth.voiced_clip_int16("dacadv-real-0", L), synth.noise_clip_int16("dacadv-real-1", L)])))
    noise = torch.from_numpy(synth.pcm_to_float(np.stack([synth.noise_clip_int16("dacadv-fake-0", L, amp=0.02), synth.noise_clip_int16("dacadv-fake-1", L, amp=0.02)])))
    return (0.8 * real + noise).unsqueeze(1), real.unsqueeze(1)


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean()) / np.sqrt((b ** 2).mean()))


def reference_error(g, name):
    """The reference's own float32 error on the fixture's input: |s32 - s64| / |s64| (relative RMS for a gradient)."""
    return (rel_rms if name in VECTORS else rel)(g[f"{name}_f32"], g[f"{name}_f64"])


def tol(g, name):
    return max(T[name], 4 * reference_error(g, name))


def error(g, name, got):
    """The device's distance from the fixture's float64 value, in the measure tol() bounds."""
    return (rel_rms if name in VECTORS else rel)(got, g[f"{name}_f64"])


def run_sequence(gen_loss, disc_loss, params, fake):
    """The recorded sequence over any implementation: gen_loss() -> (gen, feat) and disc_loss() -> 0-dim, both closed over `fake` (requires grad) and
    `params` (the discriminator's tensors, updated in place by the AdamW step here).  Returns the stored quantities as float64 / numpy."""
    out = {}
    lg, lf = gen_loss()
    (W_GEN * lg + W_FEAT * lf).backward()
    out["gen_before"], out["feat_before"], out["d_fake_before"] = float(lg.detach()), float(lf.detach()), fake.grad.detach().cpu().numpy().copy()
    fake.grad = None
    opt = torch.optim.AdamW(params, lr=LR, betas=BETAS)
    ld = disc_loss()
    opt.zero_grad()
    ld.backward()
    out["disc_loss"], out["grad_norm_d"] = float(ld.detach()), float(torch.nn.utils.clip_grad_norm_(params, CLIP_D))
    opt.step()
    assert fake.grad is None
    lg, lf = gen_loss()
    (W_GEN * lg + W_FEAT * lf).backward()
    out["gen_loss"], out["feat_loss"], out["d_fake"] = float(lg.detach()), float(lf.detach()), fake.grad.detach().cpu().numpy().copy()
    return out


def oracle_sequence(dtype=torch.float64):
    """run_sequence on the oracle's restatement of the discriminator and of GANLoss (per-clip values, averaged over the batch)."""
    from oracle import esc_oracle as O
    sd = {k: v.to(dtype).requires_grad_(True) for k, v in disc_state().items()}
    fake, real = signals()
    fake, real = fake[:, 0].to(dtype).requires_grad_(True), real[:, 0].to(dtype)
    cfg = dict(YML_DISC, bands=[tuple(b) for b in YML_DISC["bands"]])

    def gen_loss():
        lg, lf = O.gan_generator_loss(fake, real, sd, cfg)
        return lg.mean(), lf.mean()

    out = run_sequence(gen_loss, lambda: O.gan_discriminator_loss(fake, real, sd, cfg).mean(), list(sd.values()), fake)
    for k in VECTORS:
        out[k] = out[k][:, None]
    return out
