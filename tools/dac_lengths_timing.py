"""Mixed-length batches of the DAC baseline (esc.baselines.DAC, `lengths`): what a batch of clips of different lengths costs, in one process on
one GPU.  36 clips with lengths drawn once (fixed seed) between 0.5 s and 3 s at 16 kHz, DAC-Tiny and DAC-Base (name-keyed weights), `encode`
and `forward`.  Three arms alternate over --rounds rounds, each timed over a window of at least --window seconds after a warm-up:
  lengths    one call with per-clip lengths (every clip bitwise its own call)
  per_clip   one call per clip, on the clip alone (the same results)
  padded     the uniform call on the batch zero-padded to 3 s: DIFFERENT results (a clip's end sees the padded map), a cost reference only
ms per batch; padded_spread = (max - min) / min of the padded rounds is the noise a difference to that arm has to exceed.  The lengths arm is
asserted against the per-clip arm (bitwise codes) before timing.

    python tools/dac_lengths_timing.py [--clips 36] [--rounds 3] [--window 0.5] [--json OUT] > profiles/dac_lengths_timing.txt
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dac_timing as dt  # noqa: E402


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
    ap.add_argument("--models", default="dac_tiny,dac_base")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from esc import synth
    dev = torch.device("cuda:0")
    sr = 16000
    lens = np.random.RandomState(a.seed).randint(int(a.min_seconds * sr), int(a.max_seconds * sr) + 1, size=a.clips).tolist()
    Lmax = int(a.max_seconds * sr)
    pcm = np.zeros((a.clips, Lmax), np.int16)
    for i, n in enumerate(lens):
        pcm[i, :n] = (synth.voiced_clip_int16 if i % 2 else synth.noise_clip_int16)(f"dac-lengths-time-{i}", Lmax)[:n]
    x = torch.from_numpy(synth.pcm_to_float(pcm))[:, None].to(dev)
    clips = [x[b:b + 1, :, :n].contiguous() for b, n in enumerate(lens)]
    rows = []
    print(f"# python tools/dac_lengths_timing.py --clips {a.clips} --min_seconds {a.min_seconds} --max_seconds {a.max_seconds} --seed {a.seed} --rounds {a.rounds} "
          f"--warmup {a.warmup} --window {a.window}   (MI355X, one process, ms per batch of {a.clips} clips, {sum(lens)} samples in all = "
          f"{sum(lens) / (a.clips * Lmax):.3f} of the padded batch; padded_spread = (max - min) / min of the padded rounds)", flush=True)
    for name in a.models.split(","):
        m = dt.dac_model(name, dev)[0]
        with torch.no_grad():
            codes = m.encode(x, lengths=lens)[1]
            for b, c in enumerate(clips):
                c1 = m.encode(c)[1]
                assert torch.equal(codes[b:b + 1, :, :c1.shape[-1]], c1), (name, b)
        ops = {"encode": (lambda: m.encode(x, lengths=lens), lambda: [m.encode(c) for c in clips], lambda: m.encode(x)),
               "forward": (lambda: m(x, lengths=lens), lambda: [m(c) for c in clips], lambda: m(x))}
        for op, fns in ops.items():
            t = {"lengths": [], "per_clip": [], "padded": []}
            with torch.no_grad():
                for _ in range(a.rounds):
                    for arm, fn in zip(t, fns):
                        t[arm].append(window_ms(fn, a.warmup, a.window))
            mean = {k: sum(v) / len(v) for k, v in t.items()}
            spread = (max(t["padded"]) - min(t["padded"])) / min(t["padded"])
            r = {"model": name, "op": op, "precision": m.precision, "clips": a.clips, "live_fraction": round(sum(lens) / (a.clips * Lmax), 4),
                 "lengths_ms": round(mean["lengths"], 3), "per_clip_ms": round(mean["per_clip"], 3), "padded_ms": round(mean["padded"], 3),
                 "lengths_rounds": [round(v, 3) for v in t["lengths"]], "per_clip_rounds": [round(v, 3) for v in t["per_clip"]],
                 "padded_rounds": [round(v, 3) for v in t["padded"]], "padded_spread": round(spread, 4),
                 "lengths_over_padded": round(mean["lengths"] / mean["padded"], 4),
                 "slower_than_padded_beyond_spread": bool(mean["lengths"] / mean["padded"] - 1.0 > spread)}
            rows.append(r)
            print(json.dumps(r), flush=True)
        del m
        torch.cuda.empty_cache()
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
