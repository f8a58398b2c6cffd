"""TEST INFRASTRUCTURE -- input gradients of the training-mode forward: generates tests/golden/input_grad.npz by running the REAL reference
(/root/reference, imported through oracle/ref_shims.py) with name-keyed deterministic weights (esc/synth.py), in the pattern of
tools/gen_rvq_golden.py.  Run in the build container only:

    python tools/gen_input_grad_golden.py

Cases (the trainer's losses of scripts/trainer_no_adv.py:105-115 with the weights of configs/9kbps_esc_base.yaml, then loss.mean().backward()):
  x_*     x.requires_grad (tiny at S < max_streams, tiny with freeze_codebook=True, base at S = 3): x.grad
  feat_*  x_feat.requires_grad (tiny): x_feat = the reference's own STFT of x, laid out (B, F, T, 2) as codecs.py:33-34 expects: x_feat.grad
Each stores the input gradient, the codes and the per-clip losses (and x_feat itself for the spectrum cases).  Inputs are regenerated from tags by esc/synth.py.  Data only; no
reference source is stored.
"""
import json
import os
import sys

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402  (build_reference, synth, ref_shims)

WEIGHTS = dict(cm_weight=0.25, cb_weight=1.0, mel_weight=0.25, stft_weight=1.0)        # configs/9kbps_esc_base.yaml:29-33
N_SAMPLES = {"tiny": 1260, "base": 9520}                  # even frame counts; base kept short so that the fixture stays small
CASES = [("x", "tiny", 2, False), ("x", "tiny", 3, True), ("x", "base", 3, False), ("feat", "tiny", 2, False)]


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref_models = gg.ref_shims.load_reference()
    import importlib
    losses = importlib.import_module("esc.modules")
    mel_fn, stft_fn = losses.MelSpectrogramLoss(), losses.ComplexSTFTLoss()
    out = {"weights_json": np.array(json.dumps(WEIGHTS)), "n_samples_json": np.array(json.dumps(N_SAMPLES)),
           "cases_json": np.array(json.dumps(CASES))}
    models = {}
    for kind, name, S, freeze in CASES:
        if name not in models:
            cfg = gg.TINY_CFG if name == "tiny" else yaml.safe_load(open(f"{gg.ref_shims.REFERENCE_ROOT}/configs/9kbps_esc_{name}.yaml"))["model"]
            models[name] = gg.build_reference(ref_models, cfg)[0].train()
            out[f"{name}_config_json"] = np.array(json.dumps(dict(cfg)))
        model = models[name]
        model.requires_grad_(False)                          # the input gradient alone: the parameters are constants here
        tags = [f"input-grad-{name}-0", f"input-grad-{name}-1"]
        pcm = np.stack([gg.synth.noise_clip_int16(tags[0], N_SAMPLES[name]), gg.synth.voiced_clip_int16(tags[1], N_SAMPLES[name])])
        out[f"{name}_tags"] = np.array(json.dumps(tags))
        x = torch.from_numpy(gg.synth.pcm_to_float(pcm))
        if kind == "x":
            leaf = x.clone().requires_grad_(True)
            o = model(**dict(x=leaf, x_feat=None, num_streams=S, freeze_codebook=freeze))
        else:
            with torch.no_grad():
                spec = model.spec_transform(x)                       # (B, 2, F, T)
            leaf = spec.permute(0, 2, 3, 1).contiguous().requires_grad_(True)      # (B, F, T, 2): "b h w c" of codecs.py:33-34
            o = model(**dict(x=x, x_feat=leaf, num_streams=S, freeze_codebook=freeze))
        mel = mel_fn(o["raw_audio"], o["recon_audio"])
        stft = stft_fn(o["raw_feat"], o["recon_feat"])
        loss = o["cm_loss"] * WEIGHTS["cm_weight"] + o["cb_loss"] * WEIGHTS["cb_weight"] + mel * WEIGHTS["mel_weight"] + stft * WEIGHTS["stft_weight"]
        loss.mean().backward()
        tag = f"{kind}_{name}_s{S}_f{int(freeze)}"

        def vec(t):
            t = t if torch.is_tensor(t) else torch.full((x.shape[0],), float(t))
            return t.detach().numpy().astype(np.float32)
        out[f"{tag}_cm"], out[f"{tag}_cb"], out[f"{tag}_mel"], out[f"{tag}_stft"], out[f"{tag}_loss"] = vec(o["cm_loss"]), vec(o["cb_loss"]), vec(mel), vec(stft), vec(loss)
        out[f"{tag}_codes"] = o["codes"].numpy().astype(np.int16)
        out[f"{tag}_grad"] = leaf.grad.numpy().astype(np.float32)
        if kind == "feat":              # the spectrum itself: the raw-side power law is steep near zero, so the test feeds these exact values
            out[f"{tag}_xfeat"] = leaf.detach().numpy().astype(np.float32)
        print(tag, "loss", out[f"{tag}_loss"], "grad shape", leaf.grad.shape, "grad rms", float(leaf.grad.double().pow(2).mean().sqrt()))
    path = os.path.join(gg.GOLD, "input_grad.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
