"""TEST INFRASTRUCTURE -- the DAC baseline's training losses (esc.baselines.loss): generates tests/golden/dac_loss.npz by running the REAL reference
`dac/nn/loss.py` (baselines/descript of the reference repository) on the CPU in float64.  Run in the build container only; no test runs it:

    python tools/gen_dac_loss_golden.py [REFERENCE_ROOT]

The reference's `dac/__init__.py` imports audiotools (absent here), so a stub `dac` package whose __path__ points into the reference is registered, with a
stub audiotools whose AudioSignal takes its `stft` / `magnitude` / `mel_spectrogram` from the test restatement (tests/dac_loss_util.py) - the device
tools/gen_msd_golden.py uses for `resample`.

PINNED to the real reference: L1Loss and SISDRLoss entirely (they accept plain tensors), and the loss arithmetic of MelSpectrogramLoss and
MultiScaleSTFTLoss: clamp, pow, log10, the weights, the zip truncation over n_mels / mel_fmin / mel_fmax / stft_params and the batch mean.
RESTATED, NOT PINNED: audiotools' STFT (torch.stft, periodic hann, center=True, reflect padding) and librosa's Slaney filterbank - neither package is
installed where this fixture was written.

The file holds the reference signal `ref` (2 x 2049, from int16 PCM seeds of esc.synth), the estimate `est` = 1.7 x ref of the spectral cases, the estimate
`est_wave` = ref + 0.1 x noise of the two waveform losses, and per case the loss value (float64) and both gradients (float32): the yml configuration
(conf/16khz_dns_9k.yml), the class defaults, one two-scale configuration with unequal weights, the STFT loss with its defaults, the default-argument
MelSpectrogramLoss over the yml's seven windows (the zip stops after two scales), L1Loss and SISDRLoss.  Data only; no reference source is stored.
"""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "efficient-speech-codec_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
from esc import synth  # noqa: E402
import dac_loss_util as D  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
B, L = 2, 2049


def load_reference_losses(ref_root):
    at = types.ModuleType("audiotools")

    class AudioSignal:
        def __init__(self, audio_data, sample_rate=D.SR):
            self.audio_data, self.sample_rate = audio_data, sample_rate            # (B, 1, L)

        def stft(self, window_length, hop_length, window_type):
            assert window_type in (None, "hann") and hop_length == window_length // 4
            self.magnitude = D.magnitude(self.audio_data[:, 0], window_length)[:, None]            # (B, 1, F, T)

        def mel_spectrogram(self, n_mels, mel_fmin=0.0, mel_fmax=None, **kwargs):
            self.stft(**kwargs)
            nf = self.magnitude.shape[2]
            basis = torch.from_numpy(D.slaney(2 * (nf - 1), n_mels, mel_fmin, mel_fmax, self.sample_rate)).to(self.magnitude.dtype)
            return (self.magnitude.transpose(-1, 2) @ basis.T).transpose(-1, 2)

    class STFTParams:
        def __init__(self, window_length=None, hop_length=None, window_type=None, match_stride=None, padding_type=None):
            self.window_length, self.hop_length, self.window_type, self.match_stride = window_length, hop_length, window_type, match_stride

    at.AudioSignal, at.STFTParams = AudioSignal, STFTParams
    sys.modules["audiotools"] = at
    pkg = types.ModuleType("dac")
    pkg.__path__ = [os.path.join(ref_root, "baselines", "descript", "dac")]
    sys.modules["dac"] = pkg
    nn_pkg = types.ModuleType("dac.nn")
    nn_pkg.__path__ = [os.path.join(ref_root, "baselines", "descript", "dac", "nn")]
    sys.modules["dac.nn"] = nn_pkg
    return importlib.import_module("dac.nn.loss"), AudioSignal


def grads(fn, a, b):
    a = a.double().requires_grad_(True)
    b = b.double().requires_grad_(True)
    v = fn(a, b)
    v.backward()
    assert v.dim() == 0
    return np.float64(v.item()), a.grad.numpy().astype(np.float32), b.grad.numpy().astype(np.float32)


def main():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_shims
    ref_root = sys.argv[1] if len(sys.argv) > 1 else ref_shims.REFERENCE_ROOT
    mod, Signal = load_reference_losses(ref_root)
    pcm = np.stack([synth.noise_clip_int16("dac-loss-noise", L), synth.voiced_clip_int16("dac-loss-voiced", L)])
    ref = torch.from_numpy(synth.pcm_to_float(pcm))
    est = 1.7 * ref
    est_wave = ref + 0.1 * ref.std() * torch.randn(B, L, generator=torch.Generator().manual_seed(11))
    out = {"pcm": pcm, "ref": ref.numpy(), "est": est.numpy(), "est_wave": est_wave.numpy(), "readme": np.array(__doc__)}
    sig = lambda t: Signal(t[:, None])
    for name, cfg in D.CONFIGS.items():
        kw = D.module_kwargs(cfg)
        loss = (mod.MultiScaleSTFTLoss if cfg["n_mels"] is None else mod.MelSpectrogramLoss)(**kw)
        v, ga, gb = grads(lambda a, b: loss(sig(a), sig(b)), est, ref)
        out[f"{name}_loss"], out[f"{name}_d_est"], out[f"{name}_d_ref"] = v, ga, gb
        print(f"{name}: {v:.12g}")
    loss = mod.MelSpectrogramLoss(n_mels=D.YML["n_mels"], window_lengths=D.YML["window_lengths"])             # default mel_fmin / mel_fmax: two scales
    v, ga, gb = grads(lambda a, b: loss(sig(a), sig(b)), est, ref)
    out["zip_loss"], out["zip_d_est"], out["zip_d_ref"] = v, ga, gb
    v, ga, gb = grads(lambda a, b: mod.L1Loss()(a[:, None], b[:, None]), est_wave, ref)
    out["l1_loss"], out["l1_d_est"], out["l1_d_ref"] = v, ga, gb
    v, gr, ge = grads(lambda r, e: mod.SISDRLoss()(r[:, None], e[:, None]), ref, est_wave)                     # references first
    out["sisdr_loss"], out["sisdr_d_ref"], out["sisdr_d_est"] = v, gr, ge
    for scaling, zero_mean, clip_min in D.SISDR_OPTIONS:
        for reduction in ("mean", "sum"):
            m = mod.SISDRLoss(scaling=scaling, reduction=reduction, zero_mean=zero_mean, clip_min=clip_min)
            out[f"sisdr_{int(scaling)}{int(zero_mean)}{'c' if clip_min is not None else 'n'}_{reduction}"] = np.float64(m(ref.double()[:, None], est_wave.double()[:, None]).item())
    path = os.path.join(GOLD, "dac_loss.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
