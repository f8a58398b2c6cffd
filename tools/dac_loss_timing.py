"""The three losses of the DAC baseline's trainer (esc.baselines.loss: MelSpectrogramLoss and MultiScaleSTFTLoss in the configuration of
conf/16khz_dns_9k.yml, L1Loss), forward + backward with respect to the estimate, next to the float32 torch-eager restatement of the same losses
(tests/dac_loss_util.py) on the same GPU in one process: ms per evaluation of  mel(x, y) + stft(x, y) + l1(x, y); .backward()  at 16 x 3 s and 1 x 3 s (16 kHz).
The two arms alternate over --rounds rounds; a round's window runs whole evaluations, each ending in a device synchronise, until at least --window seconds
have passed, after --warmup evaluations.  The spread, (max - min) / min over an arm's rounds, is the noise a difference has to exceed.  Also printed: the
peak of torch's device allocator during one evaluation of each arm (the native arm's scratch is the library's own allocation and not in it; its size
is printed), and the native gradient against eager's.  Then the whole step of scripts/train_dac.py without the optimiser for DAC-Base and DAC-Tiny at
16 x 3 s: native losses against eager losses around the same native codec step.

    python tools/dac_loss_timing.py [--window 0.5] [--warmup 1] [--rounds 3] [--out profiles/dac_loss_timing.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "efficient-speech-codec_amd"), ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dac_loss_util as D  # noqa: E402

SAMPLES = 48000     # 3 s at 16 kHz
ARMS = ("native", "eager")


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
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


MODELS = {
    "dac_base": dict(encoder_dim=64, encoder_rates=[2, 4, 5, 8], decoder_dim=1536, decoder_rates=[8, 5, 4, 2], n_codebooks=18, codebook_size=1024,
                     codebook_dim=8, quantizer_dropout=0.5, sample_rate=16000),
    "dac_tiny": dict(encoder_dim=32, encoder_rates=[2, 4, 5, 8], decoder_dim=288, decoder_rates=[8, 5, 4, 2], n_codebooks=18, codebook_size=1024,
                     codebook_dim=8, quantizer_dropout=0.5, sample_rate=16000),
}


def step_rows(args, lines, mel, stft, l1):
    """The whole step of scripts/train_dac.py up to the optimiser (native codec forward with every parameter trainable, the three losses, the two VQ
    losses, backward) at 16 x 3 s: native losses against the eager restatement's losses around the SAME native codec step."""
    from esc import synth
    from esc.baselines import DAC
    lam = {"mel/loss": 15.0, "vq/commitment_loss": 0.25, "vq/codebook_loss": 1.0}
    lines += ["", "whole trainer step without the optimiser (scripts/train_dac.py: native codec forward + losses + backward, every parameter trainable), 16 x 3 s, ms per step;",
              "arms: native = esc.baselines.loss;  eager = the float32 torch restatement of the three losses around the same native codec step"]
    B = 16
    for name, cfg in MODELS.items():
        m = DAC(**cfg)
        m.load_state_dict({k: torch.from_numpy(synth.dac_tensor(k, tuple(v.shape))) for k, v in m.state_dict().items()}, strict=True)
        m = m.cuda().eval().set_encode_trainable("both").set_trainable("decoder")
        gen = torch.Generator().manual_seed(7)
        y = (0.1 * torch.randn(B, 1, SAMPLES, generator=gen)).cuda()
        nq = m.sample_n_quantizers(B, gen)

        def step(native):
            for p in m.parameters():
                p.grad = None
            out = m(y, n_quantizers=nq)
            a = out["audio"]
            s = y[..., :a.shape[-1]]
            d = a.detach()                    # the yml weighs the mel loss alone: the other two are reported only, as in scripts/train_dac.py
            if native:
                terms = {"mel/loss": mel(a, s), "stft/loss": stft(d, s), "waveform/loss": l1(d, s)}
            else:
                terms = {"mel/loss": D.spectral_loss(a[:, 0], s[:, 0], D.YML), "stft/loss": D.spectral_loss(d[:, 0], s[:, 0], D.STFT), "waveform/loss": D.wave_l1(d, s)}
            terms.update({"vq/commitment_loss": out["vq/commitment_loss"], "vq/codebook_loss": out["vq/codebook_loss"]})
            sum(v * terms[k] for k, v in lam.items()).backward()

        fns = {"native": lambda: step(True), "eager": lambda: step(False)}
        print(f"{name} step ...", flush=True)
        mem = {arm: peak_above(fns[arm]) for arm in ARMS}
        ms = {arm: [] for arm in ARMS}
        for _ in range(args.rounds):
            for arm in ARMS:
                ms[arm].append(timed(fns[arm], args.window, args.warmup)[0])
        first = len(lines)
        for arm in ARMS:
            v = ms[arm]
            lines.append(f"{name} {B} x 3 s   {arm:6s} losses {np.median(v):9.2f} ms   rounds {' '.join(f'{t:.2f}' for t in v)}   spread {(max(v) - min(v)) / min(v) * 100:.1f} %   "
                         f"peak memory of one step {mem[arm] / 1024:.2f} GiB")
        lines.append(f"    eager / native = {np.median(ms['eager']) / np.median(ms['native']):.3f}")
        print("\n".join(lines[first:]), flush=True)
        del m, y
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dac_loss_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no fallback"
    from esc import _native
    from esc.baselines import L1Loss, MelSpectrogramLoss, MultiScaleSTFTLoss
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    mel, stft, l1 = MelSpectrogramLoss(**D.module_kwargs(D.YML)), MultiScaleSTFTLoss(**D.module_kwargs(D.STFT)), L1Loss()
    lines = [f"the trainer's three losses (mel in the yml configuration + multi-scale STFT + waveform L1), forward + backward w.r.t. the estimate, ms per evaluation "
             f"(host clock around synchronised evaluations, windows of at least {args.window} s after {args.warmup} warm-up, {args.rounds} alternating rounds)",
             "arms: native = esc.baselines.loss;  eager = the float32 torch restatement (torch.stft, filterbank matmul, autograd)",
             f"device: {torch.cuda.get_device_name(0)}   torch {torch.__version__}", ""]
    for B in (16, 1):
        gen = torch.Generator().manual_seed(B)
        y = (0.1 * torch.randn(B, 1, SAMPLES, generator=gen)).cuda()
        x0 = (y + 0.02 * torch.randn(B, 1, SAMPLES, generator=gen).cuda())
        grads = {}

        def native():
            x = x0.clone().requires_grad_(True)
            (mel(x, y) + stft(x, y) + l1(x, y)).backward()
            grads["native"] = x.grad

        def eager():
            x = x0.clone().requires_grad_(True)
            a, b = x[:, 0], y[:, 0]
            (D.spectral_loss(a, b, D.YML) + D.spectral_loss(a, b, D.STFT) + D.wave_l1(a, b)).backward()
            grads["eager"] = x.grad

        fns = {"native": native, "eager": eager}
        print(f"{B} x 3 s ...", flush=True)
        mem = {arm: peak_above(fns[arm]) for arm in ARMS}
        diff = float((grads["native"] - grads["eager"]).norm() / grads["eager"].norm())
        ms, steps = {arm: [] for arm in ARMS}, {arm: [] for arm in ARMS}
        for _ in range(args.rounds):
            for arm in ARMS:
                t, n = timed(fns[arm], args.window, args.warmup)
                ms[arm].append(t)
                steps[arm].append(n)
        lib = _native.load()
        ws = sum(int(lib.escx_spec_loss_workspace_floats(m._handle(y.device).h, B, SAMPLES, 1, 0)) for m in (mel,)) * 4 / 2 ** 20
        ws2 = int(lib.escx_spec_loss_workspace_floats(stft._handle(y.device).h, B, SAMPLES, 1, 0)) * 4 / 2 ** 20
        first = len(lines)
        lines.append(f"{B:2d} x 3 s   |g native - eager| / |eager| = {diff:.2e} (independent noise: eager's own float32 gradient is that far from float64)   "
                     f"library scratch: mel {ws:.1f} MiB, stft {ws2:.1f} MiB (one grow-only buffer per stream, the larger of the two)")
        for arm in ARMS:
            v = ms[arm]
            lines.append(f"    {arm:6s} {np.median(v):9.3f} ms   rounds {' '.join(f'{t:.3f}' for t in v)} (evaluations {' '.join(str(n) for n in steps[arm])})   "
                         f"spread {(max(v) - min(v)) / min(v) * 100:.1f} %   peak memory of one evaluation {mem[arm]:.1f} MiB")
        med = {arm: float(np.median(ms[arm])) for arm in ARMS}
        lines.append(f"    eager / native = {med['eager'] / med['native']:.2f}")
        print("\n".join(lines[first:]), flush=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
        del y, x0
        grads.clear()
        torch.cuda.empty_cache()
    step_rows(args, lines, mel, stft, l1)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
