#!/usr/bin/env python
"""The DAC baseline's non-adversarial trainer (reference: baselines/descript/scripts/train_customize_no_adv.py:238-278) on the native path.

    python -m scripts.train_dac --config conf/16khz_dns_9k.yml --data ./train_wavs --steps 1000 --save_path ./dac_out
    python -m scripts.train_dac --synthetic dac_tiny --steps 2 --batch_size 2            # synthetic weights and clips: a smoke run

One step is the reference's train_loop: forward with the quantiser dropout, MultiScaleSTFTLoss + MelSpectrogramLoss + L1Loss on the waveform plus the two
VQ losses weighted by `lambdas`, backward, clip_grad_norm_(1e3), AdamW, ExponentialLR.  The model stays in eval mode - esc.baselines.DAC has no training
mode - with set_trainable("decoder") + set_encode_trainable("both") delivering every parameter gradient, and the dropout of nn/quantize.py:166-171 passed
as per-clip n_quantizers (DAC.sample_n_quantizers).  The codec step and the three losses (esc.baselines.loss) run in libescx.so.  Checkpoints are written
in the layout DAC.load reads: <save_path>/<tag>/dac/weights.pth with "state_dict" and "metadata": {"kwargs"}.

One departure: with the yml's decoder rates (8, 5, 4, 2) the model returns 8 samples fewer than it takes (the stride-5 block), and the losses need equal
lengths, so the signal is cut to the reconstruction's length before the losses.

Not here: wandb, the audiotools dataset and transforms, PESQ.  --data takes a directory of wav files at the model's rate (scipy), cut into random clips;
without it the clips are synthetic.  Validation reports the three losses only.
"""
import argparse
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
import numpy as np
import torch

from esc import synth
from esc.baselines import DAC, L1Loss, MelSpectrogramLoss, MultiScaleSTFTLoss

# conf/16khz_dns_9k.yml
LAMBDAS = {"mel/loss": 15.0, "adv/feat_loss": 2.0, "adv/gen_loss": 1.0, "vq/commitment_loss": 0.25, "vq/codebook_loss": 1.0}
YML_LOSSES = {"MultiScaleSTFTLoss": dict(window_lengths=[2048, 512]),
              "MelSpectrogramLoss": dict(n_mels=[5, 10, 20, 40, 80, 160, 320], window_lengths=[32, 64, 128, 256, 512, 1024, 2048], mel_fmin=[0, 0, 0, 0, 0, 0, 0],
                                         mel_fmax=[None] * 7, pow=1.0, clamp_eps=1e-5, mag_weight=0.0)}
OPTIM = {"AdamW": dict(betas=[0.8, 0.99], lr=1e-4), "ExponentialLR": dict(gamma=0.999996)}


def make_losses(cfg, sample_rate):
    """train_customize_no_adv.py:188-197."""
    return {"waveform": L1Loss(), "stft": MultiScaleSTFTLoss(sample_rate=sample_rate, **cfg["MultiScaleSTFTLoss"]),
            "mel": MelSpectrogramLoss(sample_rate=sample_rate, **cfg["MelSpectrogramLoss"])}


def train_step_losses(model, losses, signal, n_quantizers, lambdas, audio_hook=None):
    """train_loop (:251-263) up to the backward: the dict of loss values with the weighted total under "loss".  audio_hook(audio) sees the reconstruction
    (with its gradient retained) before the losses."""
    out = model(signal, model.sample_rate, n_quantizers=n_quantizers)
    recons = out["audio"]
    signal = signal[..., :recons.shape[-1]]            # decoder rates with an odd stride (the yml's 5) return a few samples fewer than they take: compare what there is
    if audio_hook is not None:
        recons.retain_grad()
        audio_hook(recons)
    # a loss without a weight is reported only (the yml weighs the mel loss alone): on the detached audio its forward computes no unit gradient
    arg = lambda k: recons if lambdas.get(k) else recons.detach()           # noqa: E731
    output = {"stft/loss": losses["stft"](arg("stft/loss"), signal), "mel/loss": losses["mel"](arg("mel/loss"), signal),
              "waveform/loss": losses["waveform"](arg("waveform/loss"), signal),
              "vq/commitment_loss": out["vq/commitment_loss"], "vq/codebook_loss": out["vq/codebook_loss"]}
    output["loss"] = sum(v * output[k] for k, v in lambdas.items() if k in output)
    return output


@torch.no_grad()
def validate(model, losses, signal):
    """val_loop (:216-235) without PESQ."""
    recons = model(signal, model.sample_rate)["audio"]
    signal = signal[..., :recons.shape[-1]]
    return {"mel/loss": float(losses["mel"](recons, signal)), "stft/loss": float(losses["stft"](recons, signal)),
            "waveform/loss": float(losses["waveform"](recons, signal))}


def save_checkpoint(model, optimizer, scheduler, save_path, tag):
    """audiotools' BaseModel.save_to_folder layout (:318-326): <save_path>/<tag>/dac/weights.pth + the extras next to it."""
    folder = os.path.join(save_path, tag, "dac")
    os.makedirs(folder, exist_ok=True)
    torch.save({"state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "metadata": {"kwargs": dict(model.kwargs)}},
               os.path.join(folder, "weights.pth"))
    torch.save(optimizer.state_dict(), os.path.join(folder, "optimizer.pth"))
    torch.save(scheduler.state_dict(), os.path.join(folder, "scheduler.pth"))
    return os.path.join(folder, "weights.pth")


class Clips:
    """(B, 1, n) float32 batches: random cuts of the wav files under `data`, or synthetic noise / voiced clips."""

    def __init__(self, data, sample_rate, n_samples, seed):
        self.rng, self.n, self.sr, self.count, self.waves = np.random.default_rng(seed), n_samples, sample_rate, 0, []
        if data:
            from scipy.io import wavfile
            for path in sorted(glob.glob(os.path.join(data, "**", "*.wav"), recursive=True)):
                sr, pcm = wavfile.read(path)
                if sr != sample_rate:
                    raise ValueError(f"{path}: {sr} Hz, the model runs at {sample_rate} Hz (resampling is out of scope)")
                x = pcm.astype(np.float32) / 32768.0 if pcm.dtype == np.int16 else pcm.astype(np.float32)
                x = x[:, 0] if x.ndim == 2 else x
                if x.size >= n_samples:
                    self.waves.append(x)
            if not self.waves:
                raise ValueError(f"no wav file of at least {n_samples} samples under {data}")

    def batch(self, B):
        clips = []
        for _ in range(B):
            if self.waves:
                w = self.waves[self.rng.integers(len(self.waves))]
                s = self.rng.integers(w.size - self.n + 1)
                clips.append(w[s:s + self.n])
            else:
                self.count += 1
                make = synth.noise_clip_int16 if self.count % 2 else synth.voiced_clip_int16
                clips.append(synth.pcm_to_float(make(f"train_dac{self.count}", self.n)))
        return torch.from_numpy(np.stack(clips)).unsqueeze(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=None, help="the reference's yml (conf/16khz_dns_9k.yml layout: DAC, AdamW, ExponentialLR, lambdas, the two loss blocks)")
    ap.add_argument("--synthetic", default=None, help="dac_syn|dac_tiny|dac_base: configuration and synthetic weights of tests/golden")
    ap.add_argument("--data", default=None, help="directory of wav files at the model's sample rate (default: synthetic clips)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--batch_size", type=int, default=None)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--duration", type=float, default=None, help="seconds per clip (default 3.0; 0.16 with --synthetic)")
    ap.add_argument("--save_path", default="./dac_output")
    ap.add_argument("--valid_freq", type=int, default=0, help="validate every this many steps (0: at the end only)")
    a = ap.parse_args()
    if bool(a.config) == bool(a.synthetic):
        ap.error("give exactly one of --config and --synthetic")
    cfg = dict(OPTIM, lambdas=dict(LAMBDAS), batch_size=16, seed=53, **YML_LOSSES)
    if a.config:
        import yaml
        cfg.update(yaml.safe_load(open(a.config)))
        model = DAC(**cfg["DAC"])
    else:
        gold = os.path.join(ROOT, "tests", "golden")
        kwargs = json.loads(str(np.load(os.path.join(gold, f"{a.synthetic}.npz"))["config_json"]))
        if not kwargs.get("quantizer_dropout"):
            kwargs["quantizer_dropout"] = 0.5             # the yml's
        model = DAC(**kwargs)
        man = json.load(open(os.path.join(gold, f"{a.synthetic}_manifest.json")))
        model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.dac_state_dict(man).items()}, strict=True)
    seed = cfg["seed"] if a.seed is None else a.seed
    B = cfg["batch_size"] if a.batch_size is None else a.batch_size
    duration = a.duration if a.duration is not None else (0.16 if a.synthetic else 3.0)
    torch.manual_seed(seed)
    model = model.to("cuda").eval()
    model.set_trainable("decoder").set_encode_trainable("both")
    losses = make_losses(cfg, model.sample_rate)
    optimizer = torch.optim.AdamW(model.parameters(), lr=cfg["AdamW"]["lr"], betas=tuple(cfg["AdamW"]["betas"]))
    scheduler = torch.optim.lr_scheduler.ExponentialLR(optimizer, cfg["ExponentialLR"]["gamma"])
    clips = Clips(a.data, model.sample_rate, int(round(duration * model.sample_rate)), seed)
    print(f"clips of {clips.n} samples from " + (f"{len(clips.waves)} wav files" if clips.waves else "the synthetic generator"), flush=True)
    gen = torch.Generator().manual_seed(seed)
    lambdas = cfg["lambdas"]
    for step in range(1, a.steps + 1):
        signal = clips.batch(B).to("cuda")
        output = train_step_losses(model, losses, signal, model.sample_n_quantizers(B, gen), lambdas)
        optimizer.zero_grad()
        output["loss"].backward()
        grad_norm = torch.nn.utils.clip_grad_norm_(model.parameters(), 1e3)
        optimizer.step()
        scheduler.step()
        print(f"step {step}  " + "  ".join(f"{k} {float(v):.6g}" for k, v in sorted(output.items())) + f"  other/grad_norm {float(grad_norm):.6g}  "
              f"other/learning_rate {optimizer.param_groups[0]['lr']:.6g}", flush=True)
        if (a.valid_freq and step % a.valid_freq == 0) or step == a.steps:
            val = validate(model, losses, clips.batch(B).to("cuda"))
            print(f"step {step}  " + "  ".join(f"test/{k} {v:.6g}" for k, v in sorted(val.items())), flush=True)
    path = save_checkpoint(model, optimizer, scheduler, a.save_path, "latest")
    print(f"saved {path}")


if __name__ == "__main__":
    main()
