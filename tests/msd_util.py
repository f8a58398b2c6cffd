"""Torch restatement of the discriminator WITH the multi-scale branch (MSD, `rates`; reference esc/models/discriminator.py:69-99), for the
tests of tests/test_msd_host.py (CPU) and tests/test_msd.py (GPU).  Works in fp32 and fp64 (the dtype of the inputs).

The period and spectrogram branches are oracle/esc_oracle.py's; this file adds the MSD: the resampler of DESIGN.md 14.1 (integer decimation,
the project's restatement of audiotools' `AudioSignal.resample` = julius `resample_frac`; neither library is installed, so that boundary is
unpinned) and seven weight-normalised Conv1d layers, four of them grouped.  tools/gen_msd_golden.py gives the reference's `AudioSignal`
stand-in THIS resampler, so the fixture pins the convolutions, their order and the losses against the real reference, not the resampler.
"""
import functools
import json
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

CFG_A = dict(rates=[1, 2, 4], periods=[3], fft_sizes=[256], sample_rate=16000, bands=[[0.0, 0.3], [0.3, 1.0]])
B_A, L_A = 3, 2001
# (kernel, stride, padding, groups) of convs.0 .. convs.5, conv_post
MSD_LAYERS = [(15, 1, 7, 1), (41, 4, 20, 4), (41, 4, 20, 16), (41, 4, 20, 64), (41, 4, 20, 256), (5, 1, 2, 1), (3, 1, 1, 1)]


def resample_taps(rate: int):
    """(taps in float64, width): 2 * width + rate taps of a Hann-windowed sinc with 24 zero crossings at the cutoff 0.945 / rate, sum 1."""
    zeros, cutoff = 24, 0.945
    width = math.ceil(zeros * rate / cutoff)
    idx = np.arange(-width, width + rate, dtype=np.float64)
    t = np.clip(idx / rate * cutoff, -zeros, zeros) * math.pi
    k = np.where(t == 0.0, 1.0, np.sin(t) / np.where(t == 0.0, 1.0, t)) * np.cos(t / zeros / 2.0) ** 2
    return k / k.sum(), width


def resample(x: torch.Tensor, rate: int) -> torch.Tensor:
    """x (B, 1, L) at sample_rate -> (B, 1, L // rate) at sample_rate / rate:  y[n] = sum_j k[j] xpad[n rate + j], xpad replicate-padded by
    (width, width + rate)."""
    if rate == 1:
        return x
    k, width = resample_taps(rate)
    xp = F.pad(x, (width, width + rate), mode="replicate")
    y = F.conv1d(xp, torch.from_numpy(k).to(x.dtype).view(1, 1, -1), stride=rate)
    return y[..., : x.shape[-1] // rate]


def msd_forward(x, sd, pfx: str, rate: int):
    """MSD.forward: x (B, 1, L), already pre-processed -> 7 feature maps (B, C, T)."""
    from oracle import esc_oracle as O
    x = resample(x, rate)
    fmap = []
    for j, (k, s, p, g) in enumerate(MSD_LAYERS):
        name = f"{pfx}convs.{j}.0." if j < 6 else f"{pfx}conv_post."
        x = F.conv1d(x, O.wn_weight(sd, name), sd[name + "bias"], stride=s, padding=p, groups=g)
        if j < 6:
            x = F.leaky_relu(x, 0.1)
        fmap.append(x)
    return fmap


def discriminator_forward(x, sd, cfg):
    """Discriminator.forward (discriminator.py:179-221): MPDs, then MSDs, then MRDs."""
    from oracle import esc_oracle as O
    x = O.disc_preprocess(x)
    out, i = [], 0
    for p in cfg["periods"]:
        out.append(O.mpd_forward(x, sd, f"discriminators.{i}.", p)); i += 1
    for r in cfg["rates"]:
        out.append(msd_forward(x, sd, f"discriminators.{i}.", r)); i += 1
    for w in cfg["fft_sizes"]:
        out.append(O.mrd_forward(x, sd, f"discriminators.{i}.", w, cfg["bands"])); i += 1
    return out


def _mean(t):
    return t.mean(dim=list(range(1, t.dim())))          # gan_loss.py's mean over [1, 2, 3]; an MSD map has two such dimensions


def gan_discriminator_loss(fake, real, sd, cfg):
    d_fake, d_real = discriminator_forward(fake.detach().unsqueeze(1), sd, cfg), discriminator_forward(real.unsqueeze(1), sd, cfg)
    loss = 0
    for xf, xr in zip(d_fake, d_real):
        loss = loss + _mean(xf[-1] ** 2) + _mean((1 - xr[-1]) ** 2)
    return loss


def gan_generator_loss(fake, real, sd, cfg):
    d_fake, d_real = discriminator_forward(fake.unsqueeze(1), sd, cfg), discriminator_forward(real.unsqueeze(1), sd, cfg)
    loss_g, loss_f = 0, 0
    for xf in d_fake:
        loss_g = loss_g + _mean((1 - xf[-1]) ** 2)
    for df, dr in zip(d_fake, d_real):
        for a, b in zip(df[:-1], dr[:-1]):
            loss_f = loss_f + _mean((a - b.detach()).abs())
    return loss_g, loss_f


def synth_state(manifest):
    """Name-keyed synthetic discriminator weights, the rule of oracle/gen_disc_golden.py synth_disc_state."""
    from esc import synth
    out = {}
    for k, shp in manifest.items():
        u = synth.hashed_uniform(k, int(np.prod(shp))).reshape(shp)
        if k.endswith("weight_v"):
            out[k] = (u / math.sqrt(int(np.prod(shp[1:])))).astype(np.float32)
        elif k.endswith("bias"):
            out[k] = (0.05 * u).astype(np.float32)
    for k, shp in manifest.items():
        if k.endswith("weight_g"):
            v = out[k[:-1] + "v"]
            nrm = np.sqrt((v.reshape(shp[0], -1).astype(np.float64) ** 2).sum(1)).reshape(shp)
            out[k] = (nrm * (1.0 + 0.5 * synth.hashed_uniform(k, int(np.prod(shp))).reshape(shp))).astype(np.float32)
    return {k: torch.from_numpy(out[k]) for k in manifest}


def clips(tag: str, B: int, L: int):
    """(real, fake) clips (B, L), the recipe of tools/gen_msd_golden.py."""
    from esc import synth
    real = torch.from_numpy(synth.pcm_to_float(np.stack([synth.voiced_clip_int16(f"{tag}-real-{i}", L) for i in range(B)])))
    noise = torch.from_numpy(synth.pcm_to_float(np.stack([synth.noise_clip_int16(f"{tag}-fake-{i}", L, amp=0.03) for i in range(B)])))
    return real, 0.7 * real + noise


def rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean()) / max(np.sqrt((b ** 2).mean()), 1e-30))


@functools.lru_cache(maxsize=None)
def fixture_a():
    """(npz, manifest, state, real, fake) of configuration A: computed once, shared by the tests, never modified."""
    from conftest import GOLDEN, load_golden
    g = load_golden("msd")
    man = json.load(open(os.path.join(GOLDEN, "msd_manifest.json")))["state_dict"]
    real, fake = clips("msd", B_A, L_A)
    return g, man, synth_state(man), real, fake
