"""Cost of the rvq+swinT training step against ESC-Base's on the same build: ms per FULL step (training forward, the trainer's four losses, backward,
FlatAdamW with clipping) on 36 clips of 47920 samples, host wall clock around synchronised steps.  Both models live in one process; after the warm-up
the arms alternate round by round (ESC, rvq, ESC, rvq, ...), each round `--steps` steps, and ESC's run-to-run spread over the rounds is printed beside the
comparison - the only comparison claimed is rvq+swinT against ESC-Base.  Also printed: escx_train_tape_bytes of both models.

    python tools/rvq_train_timing.py [--steps 5] [--rounds 4] [--warmup 3]
    python tools/rvq_train_timing.py --share        # the share of the two new kernels in the rvq step's kernel time; run under
                                                    # rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/rvq_train_timing.py --share, then
    python tools/rvq_train_timing.py --stats DIR    # reads the *_kernel_stats.csv rocprofv3 left under DIR
"""
import argparse
import csv
import glob
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

NEW_KERNELS = ("prvq_train_fwd_kernel", "prvq_train_bwd_kernel")


def rvq_model(dev):
    """The ablation yaml's model block (tests/golden/rvq_base.npz carries it) with synthetic weights."""
    from esc import synth
    from esc.models import make_model
    cfg = json.loads(str(np.load(os.path.join(ROOT, "tests", "golden", "rvq_base.npz"))["config_json"]))
    model = make_model(cfg, "rvq+swinT")
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(synth.synth_tensor(k, s))) for k, s in model._state_manifest().items() if not k.endswith(".window")})
    return model.to(dev)


def stats(folder):
    rows = []
    for f in glob.glob(os.path.join(folder, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    for key in NEW_KERNELS:
        sel = [r for r in rows if key in r["Name"]]
        ns, calls = sum(float(r["TotalDurationNs"]) for r in sel), sum(int(r["Calls"]) for r in sel)
        print(f"{key:24s} {calls:5d} dispatches  {ns / max(calls, 1) / 1e3:8.1f} us average  {100 * ns / tot:6.3f} % of kernel time")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--clips", type=int, default=36)
    ap.add_argument("--share", action="store_true")
    ap.add_argument("--stats", default=None)
    args = ap.parse_args()
    if args.stats:
        return stats(args.stats)
    from esc import _native, synth
    from esc.modules import ComplexSTFTLoss, MelSpectrogramLoss
    from esc.optim import FlatAdamW
    dev = torch.device("cuda", 0)
    pcm = np.stack([synth.noise_clip_int16(f"bench-r0-{i}", bench.TRAIN_SAMPLES) for i in range(args.clips)])
    x = torch.from_numpy(synth.pcm_to_float(pcm)).to(dev)
    mel_fn, stft_fn = MelSpectrogramLoss(), ComplexSTFTLoss()
    w = bench.TRAIN_WEIGHTS
    arms = {"rvq+swinT": rvq_model(dev).train()}
    if not args.share:
        arms = {"ESC-Base": bench.build_model(dev)[0].train(), **arms}
    opts = {k: FlatAdamW(m, lr=1e-5, max_grad_norm=0.5) for k, m in arms.items()}

    def step(name):
        model = arms[name]
        out = model(x=x, x_feat=None, num_streams=bench.NUM_STREAMS, freeze_codebook=False)
        loss = (out["cm_loss"] * w["cm_weight"] + out["cb_loss"] * w["cb_weight"] + mel_fn(out["raw_audio"], out["recon_audio"]) * w["mel_weight"]
                + stft_fn(out["raw_feat"], out["recon_feat"]) * w["stft_weight"])
        loss.mean().backward()
        opts[name].step(); opts[name].zero_grad()

    for name in arms:
        for _ in range(args.warmup):
            step(name)
    torch.cuda.synchronize(dev)
    if args.share:
        for _ in range(args.steps):
            step("rvq+swinT")
        torch.cuda.synchronize(dev)
        return
    ms = {k: [] for k in arms}
    for _ in range(args.rounds):
        for name in arms:
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step(name)
            torch.cuda.synchronize(dev)
            ms[name].append((time.perf_counter() - t0) / args.steps * 1e3)
    lib = _native.load()
    tape = {k: int(lib.escx_train_tape_bytes(m._handle(dev, for_training=True)[1])) for k, m in arms.items()}
    for k, v in ms.items():
        print(f"{k:10s} {np.mean(v):8.2f} ms / step   rounds {' '.join(f'{t:.2f}' for t in v)}   spread (max - min) {max(v) - min(v):.2f} ms   tape {tape[k] / 2 ** 30:.2f} GiB", flush=True)
    e, r = np.mean(ms["ESC-Base"]), np.mean(ms["rvq+swinT"])
    print(json.dumps({"clips": args.clips, "samples": bench.TRAIN_SAMPLES, "steps_per_round": args.steps, "rounds": args.rounds,
                      "ms_per_step": {k: round(float(np.mean(v)), 2) for k, v in ms.items()}, "esc_spread_ms": round(max(ms["ESC-Base"]) - min(ms["ESC-Base"]), 2),
                      "rvq_vs_esc_pct": round(100 * (r / e - 1), 2), "tape_bytes": tape}))


if __name__ == "__main__":
    main()
