"""The DAC baseline's stand-alone quantiser (esc.baselines.DAC: model.quantizer(z), its backward in z, its backward with the quantiser's
parameter gradients, and model.quantizer.from_latents) against the torch-eager restatement of tests/dac_encode_grad_util.py (DacRefE.quantize,
fp32, torch autograd) on the same GPU, in one process: ms per call for DAC-Base and DAC-Tiny (16 kHz configurations, name-keyed weights) at
36 x 3 s (z of 36 x 1024 x 150 for DAC-Base) and at 1 x 3 s.  z is the latent the model's own encode gives for synthetic clips.  The two arms
of a row alternate over --rounds rounds; every timed window runs for at least --window seconds (the step count is set from a first estimate),
and each arm's run-to-run spread, (max - min) / min over its rounds, is reported next to its mean: a ratio inside the spreads is no difference.
No speed is promised; the table is what was measured.

    python tools/dac_quantizer_timing.py [--rounds 3] [--window 0.5] [--out profiles/dac_quantizer_timing.txt]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import dac_encode_grad_util as eu  # noqa: E402
import dac_timing as dt  # noqa: E402


def eager_from_latents(ref, lat):
    d, zq, zp, codes = ref.cfg["codebook_dim"], 0.0, [], []
    for i in range(min(lat.shape[1] // d, ref.cfg["n_codebooks"])):
        p = f"quantizer.quantizers.{i}."
        idx = ref._codebook_search(i, lat[:, i * d:(i + 1) * d])[1]
        q = F.embedding(idx, ref.sd[p + "codebook.weight"]).transpose(1, 2)
        zp.append(q); codes.append(idx)
        zq = zq + ref._conv(q, p + "out_proj.")
    return zq, torch.cat(zp, 1), torch.stack(codes, 1)


def arms(model, ref, z):
    """{row: (native fn, eager fn)}; the backward rows include their forward."""
    wz = torch.randn_like(z)
    qkeys = [k for k in ref.sd if k.startswith("quantizer.")]
    lat = model.quantizer(z)[2]

    def loss(out):
        return (out[0] * wz).sum() + out[2].sum() + out[3]

    def native(train):
        def fn():
            model.set_encode_trainable("quantizer" if train else None)
            for p in model.parameters():
                p.grad = None
            zt = z.detach().requires_grad_(True)
            out = model.quantizer(zt)
            (loss(out) + (out[4] if train else 0.0)).backward()
        return fn

    def eager(train):
        def fn():
            for k in qkeys:
                ref.sd[k] = ref.sd[k].detach().requires_grad_(train)
            zt = z.detach().requires_grad_(True)
            out = ref.quantize(zt)
            (loss(out) + (out[4] if train else 0.0)).backward()
        return fn

    def fwd_native():
        with torch.no_grad():
            model.quantizer(z)

    def fwd_eager():
        with torch.no_grad():
            ref.quantize(z)

    def fl_native():
        model.quantizer.from_latents(lat)

    def fl_eager():
        with torch.no_grad():
            eager_from_latents(ref, lat)

    return {"forward": (fwd_native, fwd_eager), "forward+backward(z)": (native(False), eager(False)),
            "forward+backward(z, params)": (native(True), eager(True)), "from_latents": (fl_native, fl_eager)}


def window(fn, seconds):
    """ms per call over a window of at least `seconds`."""
    est = dt.timed(fn, 2, 2)
    return dt.timed(fn, max(3, math.ceil(seconds * 1e3 / max(est, 1e-3))), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dac_quantizer_timing.txt"))
    a = ap.parse_args()
    from esc import synth
    dev = torch.device("cuda:0")
    lines = [f"# python tools/dac_quantizer_timing.py --rounds {a.rounds} --window {a.window}   ({torch.cuda.get_device_name(0)}, one process; ms per call, arms alternating, "
             "windows of at least that many seconds; spread = (max - min) / min over the rounds of an arm)"]
    print(lines[0], flush=True)
    for name in ("dac_base", "dac_tiny"):
        model, sd = dt.dac_model(name, dev)
        for p in model.parameters():
            p.requires_grad_(True)
        ref = eu.DacRefE(dt.CONFIGS[name], {k: v.to(dev) for k, v in sd.items()}, torch.float32)
        for B in (36, 1):
            pcm = np.stack([synth.voiced_clip_int16(f"dac-time-{i}", 48000) if i % 2 else synth.noise_clip_int16(f"dac-time-{i}", 48000) for i in range(B)])
            with torch.no_grad():
                z = model.encode(torch.from_numpy(synth.pcm_to_float(pcm))[:, None].to(dev))[0]
            for row, (nat, eag) in arms(model, ref, z).items():
                tn, te = [], []
                for _ in range(a.rounds):
                    tn.append(window(nat, a.window))
                    te.append(window(eag, a.window))
                r = {"model": name, "z": list(z.shape), "call": row, "native_ms": round(sum(tn) / len(tn), 4), "eager_ms": round(sum(te) / len(te), 4),
                     "native_spread": round((max(tn) - min(tn)) / min(tn), 4), "eager_spread": round((max(te) - min(te)) / min(te), 4),
                     "eager_over_native": round(sum(te) / sum(tn), 2)}
                lines.append(json.dumps(r))
                print(lines[-1], flush=True)
        model.set_encode_trainable(None)
        del model, ref
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
