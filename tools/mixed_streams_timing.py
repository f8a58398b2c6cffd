"""Mixed-bitrate batches (per-clip num_streams) against the alternatives, on the bench's 36 clips of 3 s:

    uniform   every clip at S = 6 (one call)
    mixed     six clips at each S in 1..6, one call with per-clip counts (ESC.encode(x, counts), ...)
    split     the same mix as six uniform sub-batches of six clips, one call per S

Prints the driver-timed ms per step (host wall clock around `--steps` calls, synchronised) of encode, decode and eval forward, for the
default precision and bf16x3.  --profile adds the per-kernel report of one mixed forward (the clip gather / scatter launches among them).

    python tools/mixed_streams_timing.py [--steps 30] [--warmup 5] [--profile]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
import torch  # noqa: E402

import bench  # noqa: E402


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    model, _, _ = bench.build_model(dev)
    x = bench.synth_batch(36, 0).to(dev)
    counts = [1 + b % 6 for b in range(36)]                       # six clips at each S, interleaved as a service would receive them
    subs = [[b for b in range(36) if counts[b] == s] for s in range(1, 7)]
    xs = [x[idx].contiguous() for idx in subs]
    rows = []
    for mode in (model.precision, "bf16x3"):
        model.set_precision(mode)
        c6, shape = model.encode(x, 6)
        cm, _ = model.encode(x, counts)
        cs = [model.encode(xs[s - 1], s)[0] for s in range(1, 7)]
        res = {"precision": mode}
        res["encode"] = {"uniform_s6": timed(lambda: model.encode(x, 6), a.steps, a.warmup),
                         "mixed": timed(lambda: model.encode(x, counts), a.steps, a.warmup),
                         "split": timed(lambda: [model.encode(xs[s - 1], s) for s in range(1, 7)], a.steps, a.warmup)}
        res["decode"] = {"uniform_s6": timed(lambda: model.decode(c6, shape), a.steps, a.warmup),
                         "mixed": timed(lambda: model.decode(cm, shape, num_streams=counts), a.steps, a.warmup),
                         "split": timed(lambda: [model.decode(cs[s - 1], shape) for s in range(1, 7)], a.steps, a.warmup)}
        res["forward"] = {"uniform_s6": timed(lambda: model(x, None, 6), a.steps, a.warmup),
                          "mixed": timed(lambda: model(x, None, counts), a.steps, a.warmup),
                          "split": timed(lambda: [model(xs[s - 1], None, s) for s in range(1, 7)], a.steps, a.warmup)}
        for k in ("encode", "decode", "forward"):
            res[k] = {n: round(v, 3) for n, v in res[k].items()}
            print(f"{mode:7s} {k:8s} ms/step: uniform S=6 {res[k]['uniform_s6']:7.3f}   mixed {res[k]['mixed']:7.3f}   "
                  f"six sub-batches {res[k]['split']:7.3f}", flush=True)
        if a.profile:
            lib, hd = model._handle(dev)
            lib.escx_profile_enable(hd, 1)
            model(x, None, counts)
            rep = json.loads(lib.escx_profile_report(hd).decode())
            lib.escx_profile_enable(hd, 0)
            tot = sum(r["ms"] for r in rep)
            mix = {r["name"]: round(r["ms"], 4) for r in rep if r["name"].startswith("mix_") or r["name"] == "loss_reduce_streams"}
            res["profile_forward_mixed"] = {"kernel_ms": round(tot, 3), "permutation_and_loss": mix}
            print(f"{mode:7s} mixed forward kernels {tot:.3f} ms, of which {mix}", flush=True)
        rows.append(res)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
