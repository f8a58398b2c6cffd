"""Cost of the input gradient of the training-mode forward on the bench's training workload (36 clips of 3 s, ESC-Base, synthetic weights,
the trainer's four losses): ms per forward + backward, host wall clock around `--steps` synchronised steps, for three cases

    params        parameters require grad, x does not (the training step as before)
    params+input  parameters and x require grad (x.grad through the STFT adjoint, the losses' raw side included)
    input         x only: model.requires_grad_(False), the frozen-codec recipe (no parameter-gradient launch)

    python tools/input_grad_timing.py [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clips", type=int, default=36)
    args = ap.parse_args()
    from esc import synth
    from esc.modules import ComplexSTFTLoss, MelSpectrogramLoss
    dev = torch.device("cuda", 0)
    model, _, _ = bench.build_model(dev)
    model.train()
    pcm = np.stack([synth.noise_clip_int16(f"bench-r0-{i}", bench.TRAIN_SAMPLES) for i in range(args.clips)])
    x0 = torch.from_numpy(synth.pcm_to_float(pcm)).to(dev)
    mel_fn, stft_fn = MelSpectrogramLoss(), ComplexSTFTLoss()
    w = bench.TRAIN_WEIGHTS

    def step(x):
        out = model(x=x, x_feat=None, num_streams=bench.NUM_STREAMS, freeze_codebook=False)
        loss = (out["cm_loss"] * w["cm_weight"] + out["cb_loss"] * w["cb_weight"] + mel_fn(out["raw_audio"], out["recon_audio"]) * w["mel_weight"]
                + stft_fn(out["raw_feat"], out["recon_feat"]) * w["stft_weight"])
        loss.mean().backward()
        for p in model.parameters():
            p.grad = None

    res = {}
    for case in ("params", "params+input", "input"):
        model.requires_grad_(case != "input")
        x = x0.clone().requires_grad_(case != "params")
        for _ in range(args.warmup):
            step(x)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            x.grad = None
            step(x)
        torch.cuda.synchronize(dev)
        res[case] = (time.perf_counter() - t0) / args.steps * 1e3
        assert (x.grad is not None) == (case != "params")
        print(f"{case:13s} {res[case]:8.2f} ms / forward + backward", flush=True)
    print(json.dumps({"clips": args.clips, "samples": bench.TRAIN_SAMPLES, "ms": {k: round(v, 2) for k, v in res.items()},
                      "input_extra_pct": round(100 * (res["params+input"] / res["params"] - 1), 2),
                      "input_only_vs_params_pct": round(100 * (res["input"] / res["params"] - 1), 2)}))


if __name__ == "__main__":
    main()
