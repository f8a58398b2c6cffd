"""What the multi-scale branch (MSD, `Discriminator(rates=[...])`) costs in the adversarial step: the discriminator's share of one step -
one forward over [reconstruction | real] (GANLoss.adversarial_forward), the generator losses' backward to the waveform, the discriminator
loss and its parameter gradients - at 36 x 3 s (72 clips of 48000 samples, 16 kHz), default periods / fft sizes, `rates=[]` against
`rates=[1, 2, 4]`.  The two arms alternate over --rounds rounds in one process with the same warm-up and step counts; every step ends in a
device synchronise inside the host-clock window.  The spread, (max - min) / min over an arm's rounds, is the noise a difference has to
exceed.  Also printed: the per-layer device times of the MSD sub-discriminators from the library's per-launch profile (one extra step with a
stream synchronise after every launch group - a breakdown, not a step time).

    python tools/msd_timing.py [--steps 3] [--warmup 1] [--rounds 3] [--clips 36] [--out profiles/msd_timing.txt]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

ARMS = {"rates=[]": [], "rates=[1,2,4]": [1, 2, 4]}
L = 48000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--clips", type=int, default=36)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msd_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no fallback"
    from esc import _native
    from esc.models import Discriminator
    from esc.modules import GANLoss
    B = args.clips
    gen = torch.Generator().manual_seed(0)
    real = (0.3 * torch.randn(B, L, generator=gen)).cuda()
    fake = (real + 0.03 * torch.randn(B, L, generator=gen).cuda())
    gans = {}
    for name, rates in ARMS.items():
        torch.manual_seed(1)
        gans[name] = GANLoss(Discriminator(rates=rates, sample_rate=16000).cuda())

    def step(gan):
        disc = gan.discriminator
        for p in disc.parameters():
            p.grad = None
        fg = fake.clone().requires_grad_(True)
        d_fake, d_real = gan.adversarial_forward(fg, real)
        lg, lf = gan.generator_loss_from(d_fake, d_real)
        (lg + 2.0 * lf).mean().backward()
        gan.discriminator_backward_from(d_fake, d_real)

    def timed(gan):
        for _ in range(args.warmup):
            step(gan)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step(gan)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    lines = [f"discriminator forward + backward of one adversarial step, {B} x 3 s over [reconstruction | real] = {2 * B} clips of {L} samples, default "
             f"periods / fft sizes, precision 'split'",
             f"ms per step (host clock around {args.steps} synchronised steps, {args.warmup} warm-up, {args.rounds} alternating rounds)",
             f"device: {torch.cuda.get_device_name(0)}   torch {torch.__version__}", ""]
    ms = {name: [] for name in ARMS}
    for _ in range(args.rounds):
        for name in ARMS:
            ms[name].append(timed(gans[name]))
    for name in ARMS:
        v = ms[name]
        lines.append(f"    {name:14s} {np.median(v):9.2f} ms   rounds {' '.join(f'{x:.2f}' for x in v)}   spread {(max(v) - min(v)) / min(v) * 100:.1f} %")
    a, b = (float(np.median(ms[n])) for n in ARMS)
    lines.append(f"    three MSDs add {b - a:.2f} ms = {100 * (b - a) / a:.1f} % of the discriminator's share without them")
    # per-layer device times of the MSD sub-discriminators (discriminators.5 .. 7 with the default five periods)
    lib = _native.load()
    _native.check(lib.escx_disc_profile_enable(1))
    step(gans["rates=[1,2,4]"])
    torch.cuda.synchronize()
    rows = json.loads(lib.escx_disc_profile_report().decode())
    _native.check(lib.escx_disc_profile_enable(0))
    lines += ["", "per-layer device time of the MSD layers in one profiled step (launches serialised; fwd covers the 72 clips, dX the 36 reconstructions and then "
              "all 72, dW the 72):"]
    tot = {}
    for r in rows:
        name = r["name"]
        if any(f"discriminators.{i}." in name for i in (5, 6, 7)):
            kind, layer = name.split("[")[0], name.split("[")[1].rstrip("]").split(".", 2)[2]
            k = (kind, layer)
            t = tot.setdefault(k, [0.0, 0.0, 0]); t[0] += r["ms"]; t[1] += r["flops"]; t[2] += r["calls"]
    for (kind, layer), (t, fl, calls) in tot.items():
        lines.append(f"    {kind:5s} {layer:14s} {t:8.3f} ms over the three rates ({calls} launch groups)   {fl / (t * 1e9):7.1f} TFLOP/s (useful FLOPs)")
    lines.append(f"    all MSD layers {sum(t for t, _, _ in tot.values()):.2f} ms")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
    print("wrote", args.out)


if __name__ == "__main__":
    main()
