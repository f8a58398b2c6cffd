"""One whole-model training step of the DAC baseline, forward + backward of a waveform MSE with every parameter trainable
(esc.baselines.DAC.set_encode_trainable("both") + set_trainable("decoder"): include/escx.h escx_dac_encode_tape /
escx_dac_encode_backward_params, escx_dac_decode_tape / escx_dac_decode_backward_params), next to torch-eager autograd of the restatement
(tests/dac_encode_grad_util.DacRefE.forward_dict, the reference's straight-through quantiser) with every parameter requiring a gradient, on the
same GPU in one process: ms per step of  loss = mse(forward(x)["audio"], x cut to the audio's length); loss.backward()  for DAC-Base and DAC-Tiny at 36 x 3 s and 1 x 3 s
(16 kHz).  The two arms alternate over --rounds rounds; a round's window runs whole steps, each ending in a device synchronise, until at least
--window seconds have passed, after --warmup steps.  The spread, (max - min) / min over an arm's rounds, is the noise a difference has to exceed.
Also printed: the peak of torch's device allocator during one step of each arm (the handle's scratch and its parameter-gradient workspaces are its
own allocations and not in it; the workspaces' size is printed), and the native gradients against eager's.  No optimiser step: its cost is the
same in both arms.

    python tools/dac_train_timing.py [--window 0.5] [--warmup 1] [--rounds 3] [--out profiles/dac_train_timing.txt]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dac_encode_grad_util as eu  # noqa: E402
from esc import synth  # noqa: E402

CONFIGS = {
    "dac_base": dict(encoder_dim=64, encoder_rates=[2, 4, 5, 8], decoder_dim=1536, decoder_rates=[8, 5, 4, 2], n_codebooks=18, codebook_size=1024,
                     codebook_dim=8, sample_rate=16000),
    "dac_tiny": dict(encoder_dim=32, encoder_rates=[2, 4, 5, 8], decoder_dim=288, decoder_rates=[8, 5, 4, 2], n_codebooks=18, codebook_size=1024,
                     codebook_dim=8, sample_rate=16000),
}
SAMPLES = 48000     # 3 s at 16 kHz
ARMS = ("native", "eager")


def timed(fn, window, warmup):
    """(ms per step, steps) over whole synchronised steps until `window` seconds have passed."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dac_train_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no fallback"
    from esc.baselines import DAC
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = [f"whole-model training step (forward + backward of a waveform MSE, every parameter trainable), ms per step (host clock around synchronised steps, "
             f"windows of at least {args.window} s after {args.warmup} warm-up, {args.rounds} alternating rounds)",
             "arms: native = esc.baselines.DAC with set_encode_trainable('both') + set_trainable('decoder');  eager = torch autograd of the restatement",
             f"device: {torch.cuda.get_device_name(0)}   torch {torch.__version__}", ""]
    for name, cfg in CONFIGS.items():
        m = DAC(**cfg)
        sd = {k: torch.from_numpy(synth.dac_tensor(k, tuple(v.shape))) for k, v in m.state_dict().items()}
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval().set_encode_trainable("both").set_trainable("decoder")
        named = dict(m.named_parameters())
        for p in named.values():
            p.requires_grad_(True)
        ref = eu.DacRefE(cfg, {k: v.cuda() for k, v in sd.items()}, torch.float32)
        leaves = {k: ref.sd[k].requires_grad_(True) for k in named}
        lib, hd = m._handle(torch.device("cuda:0"))
        for B in (36, 1):
            gen = torch.Generator().manual_seed(B)
            x = (0.5 * torch.randn(B, 1, SAMPLES, generator=gen)).clamp(-1, 1).cuda()
            grads = {}

            def native():
                for p in named.values():
                    p.grad = None
                a = m(x)["audio"]                             # these rates return a few samples fewer than they take (the stride-5 block)
                (a - x[..., :a.shape[-1]]).pow(2).mean().backward()
                grads["native"] = {k: p.grad for k, p in named.items()}

            def eager():
                for p in leaves.values():
                    p.grad = None
                a = ref.forward_dict(x)["audio"]
                (a - x[..., :a.shape[-1]]).pow(2).mean().backward()
                grads["eager"] = {k: p.grad for k, p in leaves.items()}

            fns = {"native": native, "eager": eager}
            print(f"{name} {B} x 3 s ...", flush=True)
            mem = {arm: peak_above(fns[arm]) for arm in ARMS}
            # the codebooks are off this loss's graph (the straight-through estimator detaches them): eager leaves None, native writes zeros
            on = [k for k in named if grads["eager"][k] is not None]
            off = [k for k in named if grads["eager"][k] is None]
            assert all(k.endswith("codebook.weight") and not bool(grads["native"][k].any()) for k in off)
            diff = max(float((grads["native"][k] - grads["eager"][k]).norm() / grads["eager"][k].norm()) for k in on)
            grads.clear()
            ms, steps = {arm: [] for arm in ARMS}, {arm: [] for arm in ARMS}
            for _ in range(args.rounds):
                for arm in ARMS:
                    t, n = timed(fns[arm], args.window, args.warmup)
                    ms[arm].append(t)
                    steps[arm].append(n)
            ws = int(lib.escx_dac_param_grad_workspace_floats(hd))
            first = len(lines)
            lines.append(f"{name} {B:2d} x 3 s   worst tensor |g native - eager| / |eager| = {diff:.2e} (the two arms choose their codes independently)   "
                         f"parameter-gradient workspaces {ws * 4 / 2 ** 20:.1f} MiB")
            for arm in ARMS:
                v = ms[arm]
                lines.append(f"    {arm:6s} {np.median(v):9.2f} ms   rounds {' '.join(f'{t:.2f}' for t in v)} (steps {' '.join(str(n) for n in steps[arm])})   "
                             f"spread {(max(v) - min(v)) / min(v) * 100:.1f} %   peak memory of one step {mem[arm]:.2f} GiB")
            med = {arm: float(np.median(ms[arm])) for arm in ARMS}
            lines.append(f"    eager / native = {med['eager'] / med['native']:.2f}")
            print("\n".join(lines[first:]), flush=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
            grads.clear()
            for p in list(named.values()) + list(leaves.values()):
                p.grad = None
            del x
            torch.cuda.empty_cache()
        del m, ref, leaves, named
        torch.cuda.empty_cache()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
