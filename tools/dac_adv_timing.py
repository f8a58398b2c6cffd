"""One adversarial training step of the DAC baseline next to one non-adversarial step, both built from scripts/train_dac.py's own functions with the
optimisers included (train_step_losses, backward, clip_grad_norm_, AdamW, ExponentialLR; the adversarial arm adds discriminator_update and
GANLoss.generator_loss over the yml's discriminator), on one GPU in one process: ms per step for DAC-Tiny and DAC-Base at 16 x 3 s (16 kHz), the yml's batch.
The two arms alternate over --rounds rounds; a round's window runs whole steps, each ending in a device synchronise, until at least --window seconds have
passed, after --warmup steps.  The spread, (max - min) / min over an arm's rounds, is the noise a difference has to exceed.  Also printed: the peak of
torch's device allocator during one step of each arm (the native handles' scratch is their own allocation and not in it).  The parent has no adversarial step:
no speed is compared with one.

    python tools/dac_adv_timing.py [--window 0.5] [--warmup 1] [--rounds 3] [--out profiles/dac_adv_timing.txt]
    python tools/dac_adv_timing.py --steps 3 --only dac_tiny --arm adv          # a few bare steps and nothing else: what a kernel trace wraps
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from esc import synth  # noqa: E402

CONFIGS = {
    "dac_tiny": dict(encoder_dim=32, encoder_rates=[2, 4, 5, 8], decoder_dim=288, decoder_rates=[8, 5, 4, 2], n_codebooks=18, codebook_size=1024,
                     codebook_dim=8, sample_rate=16000, quantizer_dropout=0.5),
    "dac_base": dict(encoder_dim=64, encoder_rates=[2, 4, 5, 8], decoder_dim=1536, decoder_rates=[8, 5, 4, 2], n_codebooks=18, codebook_size=1024,
                     codebook_dim=8, sample_rate=16000, quantizer_dropout=0.5),
}
B, SAMPLES = 16, 48000
ARMS = ("adv", "no-adv")


def timed(fn, window, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while True:
        fn()
        torch.cuda.synchronize()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= window:
            return dt / n * 1e3, n


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 30


def make_arm(T, cfg, adv):
    """A closure running one whole step of the script: its own model, optimisers and (adv) discriminator."""
    from esc.baselines import DAC, Discriminator, GANLoss
    m = DAC(**cfg)
    m.load_state_dict({k: torch.from_numpy(synth.dac_tensor(k, tuple(v.shape))) for k, v in m.state_dict().items()}, strict=True)
    m = m.cuda().eval().set_trainable("decoder").set_encode_trainable("both")
    losses = T.make_losses(T.YML_LOSSES, m.sample_rate)
    kw = dict(lr=T.OPTIM["AdamW"]["lr"], betas=tuple(T.OPTIM["AdamW"]["betas"]))
    opt = torch.optim.AdamW(m.parameters(), **kw)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, T.OPTIM["ExponentialLR"]["gamma"])
    pack = None
    if adv:
        disc = Discriminator(**T.YML_DISCRIMINATOR).cuda()
        opt_d = torch.optim.AdamW(disc.parameters(), **kw)
        pack = (GANLoss(disc), opt_d, torch.optim.lr_scheduler.ExponentialLR(opt_d, T.OPTIM["ExponentialLR"]["gamma"]))
    gen = torch.Generator().manual_seed(53)
    x = (0.5 * torch.randn(B, 1, SAMPLES, generator=gen)).clamp(-1, 1).cuda()

    def step():
        out = T.train_step_losses(m, losses, x, m.sample_n_quantizers(B, gen), T.LAMBDAS, adv=pack)
        opt.zero_grad()
        out["loss"].backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 1e3)
        opt.step()
        sched.step()
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dac_adv_timing.txt"))
    ap.add_argument("--steps", type=int, default=0, help="run this many bare steps of --arm on --only and exit (for a kernel trace)")
    ap.add_argument("--only", default=None, choices=sorted(CONFIGS))
    ap.add_argument("--arm", default="adv", choices=ARMS)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no fallback"
    from scripts import train_dac as T
    if args.steps:
        step = make_arm(T, CONFIGS[args.only or "dac_tiny"], args.arm == "adv")
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = [f"one training step of scripts/train_dac.py's functions, optimisers included, {B} x 3 s at 16 kHz, ms per step (host clock around synchronised steps, "
             f"windows of at least {args.window} s after {args.warmup} warm-up, {args.rounds} alternating rounds)",
             "arms: adv = --adv (discriminator update, then the generator's losses with the updated discriminator);  no-adv = the step without --adv",
             f"device: {torch.cuda.get_device_name(0)}   torch {torch.__version__}", ""]
    for name, cfg in CONFIGS.items():
        if args.only and name != args.only:
            continue
        fns = {"adv": make_arm(T, cfg, True), "no-adv": make_arm(T, cfg, False)}
        print(f"{name} {B} x 3 s ...", flush=True)
        for arm in ARMS:
            fns[arm]()                             # the first step creates the handles' scratch and the optimisers' state
        mem = {arm: peak_above(fns[arm]) for arm in ARMS}
        ms, steps = {arm: [] for arm in ARMS}, {arm: [] for arm in ARMS}
        for _ in range(args.rounds):
            for arm in ARMS:
                t, n = timed(fns[arm], args.window, args.warmup)
                ms[arm].append(t)
                steps[arm].append(n)
        first = len(lines)
        lines.append(f"{name} {B} x 3 s")
        for arm in ARMS:
            v = ms[arm]
            lines.append(f"    {arm:6s} {np.median(v):9.2f} ms   rounds {' '.join(f'{t:.2f}' for t in v)} (steps {' '.join(str(n) for n in steps[arm])})   "
                         f"spread {(max(v) - min(v)) / min(v) * 100:.1f} %   peak memory of one step {mem[arm]:.2f} GiB")
        med = {arm: float(np.median(ms[arm])) for arm in ARMS}
        lines.append(f"    adv / no-adv = {med['adv'] / med['no-adv']:.2f}   (adv - no-adv = {med['adv'] - med['no-adv']:.2f} ms: two discriminator passes of {2 * B} clips, "
                     f"their backwards and the discriminator's optimiser)")
        print("\n".join(lines[first:]), flush=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        del fns
        torch.cuda.empty_cache()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
