"""Mixed-length batches of esc.ESC (`lengths`): what a batch of clips of different lengths costs, in one process on one GPU.  ESC-Base (name-keyed
synthetic weights), 36 clips with lengths drawn once (fixed seed) between 0.5 s and 3 s at 16 kHz and snapped down to valid ones (a multiple of
4 hops: the latent width is then a multiple of `overlap`), `encode` and the eval `forward` at 6 streams, in the default precision and in fp32.
Three arms alternate over --rounds rounds, each timed over a window of at least --window seconds after a warm-up:
  lengths    one call with per-clip lengths (every clip gets its own answer)
  per_clip   one plain call per clip, on the clip alone (the same answers)
  padded     the plain call on the batch zero-padded to 3 s: DIFFERENT results (ESC is not local in time), a cost reference only
ms per batch; *_spread = (max - min) / min of that arm's rounds is the noise a difference between arms has to exceed.  The lengths arm runs the
padded maps (B, H * Wmax, C): its row-wise kernels also process the tokens past each clip's end, so it cannot beat the padded arm by much;
live_fraction is the share of the padded batch's samples that belong to a clip.  Before timing, the lengths arm's codes are compared with the
per-clip arm's and the number that differ is reported (the launch heuristics of the plain call depend on the clip's own token count, so a
near-tie may resolve the other way; tests/test_esc_lengths.py holds the parity contract).

    python tools/esc_lengths_timing.py [--clips 36] [--rounds 3] [--window 0.5] [--json OUT] > profiles/esc_lengths_timing.txt
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def window_ms(fn, warmup, window):
    """ms per call over a window of at least `window` seconds (at least 3 calls), after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        if n >= 3:
            torch.cuda.synchronize()
            if time.perf_counter() - t0 >= window:
                return (time.perf_counter() - t0) / n * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=36)
    ap.add_argument("--min_seconds", type=float, default=0.5)
    ap.add_argument("--max_seconds", type=float, default=3.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--streams", type=int, default=6)
    ap.add_argument("--precisions", default="default,fp32")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from esc import synth
    from gpu_util import build_models
    dev = torch.device("cuda:0")
    sr = 16000
    model = build_models("base")[0]
    snap = 4 * model.hop_length                 # L = 4 m hops -> 4 m + 1 frames -> 2 m latent frames
    Lmax = int(a.max_seconds * sr) // snap * snap
    lens = [int(n) // snap * snap for n in np.random.RandomState(a.seed).randint(int(a.min_seconds * sr), int(a.max_seconds * sr) + 1, size=a.clips)]
    pcm = np.zeros((a.clips, Lmax), np.int16)
    for i, n in enumerate(lens):
        pcm[i, :n] = (synth.voiced_clip_int16 if i % 2 else synth.noise_clip_int16)(f"esc-lengths-time-{i}", Lmax)[:n]
    x = torch.from_numpy(synth.pcm_to_float(pcm)).to(dev)
    clips = [x[b:b + 1, :n].contiguous() for b, n in enumerate(lens)]
    S, ov = a.streams, model.cfg["overlap"]
    widths = model.frame_lengths(lens)
    rows = []
    print(f"# python tools/esc_lengths_timing.py --clips {a.clips} --min_seconds {a.min_seconds} --max_seconds {a.max_seconds} --seed {a.seed} --rounds {a.rounds} "
          f"--warmup {a.warmup} --window {a.window} --streams {S}   (MI355X, ESC-Base, one process, ms per batch of {a.clips} clips, {sum(lens)} samples in all = "
          f"{sum(lens) / (a.clips * Lmax):.3f} of the padded batch; <arm>_spread = (max - min) / min of the arm's rounds)", flush=True)
    for prec in a.precisions.split(","):
        if prec != "default":
            model.set_precision(prec)
        with torch.no_grad():
            codes = model.encode(x, S, lengths=lens)[0]
            differ = 0
            for b, c in enumerate(clips):
                c1 = model.encode(c, S)[0]
                differ += int((codes[b:b + 1, :, :, :widths[b] // ov] != c1).sum())
        fwd = lambda t, **k: model(**dict(x=t, x_feat=None, num_streams=S, **k))
        ops = {"encode": (lambda: model.encode(x, S, lengths=lens), lambda: [model.encode(c, S) for c in clips], lambda: model.encode(x, S)),
               "forward": (lambda: fwd(x, lengths=lens), lambda: [fwd(c) for c in clips], lambda: fwd(x))}
        for op, fns in ops.items():
            t = {"lengths": [], "per_clip": [], "padded": []}
            with torch.no_grad():
                for _ in range(a.rounds):
                    for arm, fn in zip(t, fns):
                        t[arm].append(window_ms(fn, a.warmup, a.window))
            mean = {k: sum(v) / len(v) for k, v in t.items()}
            spread = {k: (max(v) - min(v)) / min(v) for k, v in t.items()}
            r = {"model": "base", "op": op, "precision": model.precision, "clips": a.clips, "live_fraction": round(sum(lens) / (a.clips * Lmax), 4),
                 "codes_differing_from_per_clip_calls": differ,
                 "lengths_ms": round(mean["lengths"], 3), "per_clip_ms": round(mean["per_clip"], 3), "padded_ms": round(mean["padded"], 3),
                 "lengths_rounds": [round(v, 3) for v in t["lengths"]], "per_clip_rounds": [round(v, 3) for v in t["per_clip"]],
                 "padded_rounds": [round(v, 3) for v in t["padded"]],
                 "lengths_spread": round(spread["lengths"], 4), "per_clip_spread": round(spread["per_clip"], 4), "padded_spread": round(spread["padded"], 4),
                 "lengths_over_per_clip": round(mean["lengths"] / mean["per_clip"], 4), "lengths_over_padded": round(mean["lengths"] / mean["padded"], 4)}
            rows.append(r)
            print(json.dumps(r), flush=True)
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
