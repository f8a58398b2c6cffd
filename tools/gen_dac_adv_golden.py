"""TEST INFRASTRUCTURE -- the DAC baseline's adversarial step (esc.baselines.GANLoss, scripts/train_dac.py --adv): generates tests/golden/dac_adv.npz by
running the REAL reference `dac.nn.loss.GANLoss` over the REAL `dac.model.discriminator.Discriminator` (baselines/descript of the reference repository) on
the CPU, once in float64 and once in float32.  Run in the build container only; no test runs it:

    python tools/gen_dac_adv_golden.py [REFERENCE_ROOT]

The reference's `dac/__init__.py` imports audiotools (absent here), so stub `dac`, `dac.nn` and `dac.model` packages whose __path__ point into the reference
are registered, with a stub audiotools: `ml.BaseModel` = nn.Module and an AudioSignal that carries `.audio_data`, `.clone()`, `.detach()` and `.stft()`.
PINNED to the real reference: every convolution, weight normalisation, the pre-processing, the period reshape, the band split, both GAN losses and the
feature-matching loss.  RESTATED, NOT PINNED: audiotools' matched-stride STFT (as in tests/golden/disc.npz and oracle/gen_disc_golden.py).

Inputs and sequence: tests/dac_adv_util.py (the yml's discriminator filled from tests/golden/disc_manifest.json, two clips of 2552 samples; generator losses
before the update, the discriminator's loss / backward / clip_grad_norm_(10) / one AdamW step, generator losses and d (gen + 2 feat) / d fake after it).
Stored per dtype (`_f64`, `_f32`): disc_loss, grad_norm_d, gen_before, feat_before, gen_loss, feat_loss, d_fake_before, d_fake (gradients as float32
copies), and the float64 scalars of the oracle's restatement (`oracle_*`).  Asserted here and again by tests/test_dac_adv_host.py: the restatement agrees with
the reference on every scalar, and each after-update loss is at least 100 GPU-test tolerances from its before-update value.  Data only; no reference source is
stored.
"""
import importlib
import math
import os
import sys
import types

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (os.path.join(ROOT, "efficient-speech-codec_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import dac_adv_util as A  # noqa: E402


def load_reference(ref_root):
    at, ml = types.ModuleType("audiotools"), types.ModuleType("audiotools.ml")

    class STFTParams:
        def __init__(self, window_length=None, hop_length=None, window_type=None, match_stride=None, padding_type=None):
            self.window_length, self.hop_length, self.window_type, self.match_stride, self.padding_type = window_length, hop_length, window_type, match_stride, padding_type

    class AudioSignal:
        def __init__(self, audio_data, sample_rate=16000, stft_params=None):
            self.audio_data, self.sample_rate, self.stft_params = audio_data, sample_rate, stft_params

        def clone(self):
            return AudioSignal(self.audio_data.clone(), self.sample_rate, self.stft_params)

        def detach(self):
            return AudioSignal(self.audio_data.detach(), self.sample_rate, self.stft_params)

        def stft(self):
            p, x = self.stft_params, self.audio_data
            wl, hop = p.window_length, p.hop_length
            assert p.match_stride and hop == wl // 4
            right, pad = math.ceil(x.shape[-1] / hop) * hop - x.shape[-1], (wl - hop) // 2
            xp = torch.nn.functional.pad(x, (pad, pad + right), "reflect")
            s = torch.stft(xp.reshape(-1, xp.shape[-1]), n_fft=wl, hop_length=hop, window=torch.hann_window(wl, dtype=x.dtype), return_complex=True, center=True)
            return s.reshape(x.shape[0], x.shape[1], s.shape[-2], s.shape[-1])[..., 2:-2]

    ml.BaseModel = nn.Module
    at.AudioSignal, at.STFTParams, at.ml = AudioSignal, STFTParams, ml
    sys.modules["audiotools"], sys.modules["audiotools.ml"] = at, ml
    base = os.path.join(ref_root, "baselines", "descript", "dac")
    for name, path in (("dac", base), ("dac.nn", os.path.join(base, "nn")), ("dac.model", os.path.join(base, "model"))):
        pkg = types.ModuleType(name)
        pkg.__path__ = [path]
        sys.modules[name] = pkg
    return importlib.import_module("dac.nn.loss").GANLoss, importlib.import_module("dac.model.discriminator").Discriminator, AudioSignal


def reference_sequence(GANLoss, Discriminator, Signal, dtype):
    disc = Discriminator(**A.YML_DISC)
    disc.load_state_dict(A.disc_state(), strict=True)
    disc = disc.to(dtype)
    gan = GANLoss(disc)
    fake, real = A.signals()
    fake, real = fake.to(dtype).requires_grad_(True), real.to(dtype)
    return A.run_sequence(lambda: gan.generator_loss(Signal(fake), Signal(real)), lambda: gan.discriminator_loss(Signal(fake), Signal(real)),
                          list(disc.parameters()), fake)


def check(out):
    """The two conditions the GPU tests rest on (tests/test_dac_adv_host.py repeats them from the file)."""
    for k in A.SCALARS:
        assert A.rel(out[f"oracle_{k}_f64"], out[f"{k}_f64"]) <= A.RESTATEMENT_RTOL, k
    for after, before in (("gen_loss", "gen_before"), ("feat_loss", "feat_before")):
        change = A.rel(out[f"{after}_f64"], out[f"{before}_f64"])
        assert change >= A.MIN_CHANGE * A.tol(out, after), (after, change, A.tol(out, after))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_shims
    ref_root = sys.argv[1] if len(sys.argv) > 1 else ref_shims.REFERENCE_ROOT
    GANLoss, Discriminator, Signal = load_reference(ref_root)
    out = {"readme": np.array(__doc__)}
    for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        for k, v in reference_sequence(GANLoss, Discriminator, Signal, dtype).items():
            out[f"{k}_{tag}"] = v.astype(np.float32) if k in A.VECTORS else np.float64(v)
    for k, v in A.oracle_sequence(torch.float64).items():
        if k in A.SCALARS:
            out[f"oracle_{k}_f64"] = np.float64(v)
    for k in A.SCALARS + A.VECTORS:
        print(f"{k:14s} f64 {np.linalg.norm(out[f'{k}_f64']):.9g}   float32 error {A.reference_error(out, k):.2e}   GPU-test bound {A.tol(out, k):.2e}"
              + (f"   oracle {A.rel(out[f'oracle_{k}_f64'], out[f'{k}_f64']):.1e}" if k in A.SCALARS else ""))
    check(out)
    path = os.path.join(A.GOLDEN, "dac_adv.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
