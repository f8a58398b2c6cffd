"""Decode forward + backward of the DAC baseline with the decoder's parameter gradients (esc.baselines.DAC.set_trainable("decoder"):
include/escx.h escx_dac_decode_tape / escx_dac_decode_backward_params) next to the latent-only native backward (escx_dac_decode_backward) and to
torch-eager autograd of the restatement (tests/dac_util.DacRef.decoder) with the decoder's parameters requiring gradients, on the same GPU in
one process: ms per step of  audio = decode(z); (audio * w).sum().backward()  with z requiring a gradient in every arm, for DAC-Base and
DAC-Tiny at 36 x 3 s and 1 x 3 s (16 kHz, 150 frames).  The three arms alternate over --rounds rounds with the same warm-up and step counts;
every step ends in a device synchronise inside the host-clock window.  The spread, (max - min) / min over an arm's rounds, is the noise a
difference has to exceed.  Also printed: the peak of torch's device allocator during one step of each arm (the handle's scratch and its
parameter-gradient workspace are its own allocations and not in it; the workspace's size is printed), and the native parameter gradients
against eager's.

    python tools/dac_param_grad_timing.py [--steps 3] [--warmup 1] [--rounds 3] [--out profiles/dac_param_grad_timing.txt]
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

import dac_util as du  # noqa: E402
from esc import synth  # noqa: E402

CONFIGS = {
    "dac_base": dict(encoder_dim=64, encoder_rates=[2, 4, 5, 8], decoder_dim=1536, decoder_rates=[8, 5, 4, 2], n_codebooks=18, codebook_size=1024,
                     codebook_dim=8, sample_rate=16000),
    "dac_tiny": dict(encoder_dim=32, encoder_rates=[2, 4, 5, 8], decoder_dim=288, decoder_rates=[8, 5, 4, 2], n_codebooks=18, codebook_size=1024,
                     codebook_dim=8, sample_rate=16000),
}
FRAMES = 150        # 3 s at 16 kHz, hop 320
ARMS = ("params", "latent", "eager")


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dac_param_grad_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no fallback"
    from esc.baselines import DAC
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    lines = [f"decode forward + backward, ms per step (host clock around {args.steps} synchronised steps, {args.warmup} warm-up, {args.rounds} alternating rounds)",
             "arms: params = native, decoder parameter gradients + d_z;  latent = native, d_z only;  eager = torch autograd of the restatement, decoder "
             "parameter gradients + d_z",
             f"device: {torch.cuda.get_device_name(0)}   torch {torch.__version__}", ""]
    for name, cfg in CONFIGS.items():
        m = DAC(**cfg)
        sd = {k: torch.from_numpy(synth.dac_tensor(k, tuple(v.shape))) for k, v in m.state_dict().items()}
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval()
        dec = {k: p for k, p in m.named_parameters() if k.startswith("decoder.")}
        for k, p in m.named_parameters():
            p.requires_grad_(k in dec)
        ref = du.DacRef(cfg, {k: v.cuda() for k, v in sd.items()})
        leaves = {k: ref.sd[k].requires_grad_(True) for k in dec}
        lib, hd = m._handle(torch.device("cuda:0"))
        ws = int(lib.escx_dac_param_grad_workspace_floats(hd))
        lines.append(f"{name}: parameter-gradient workspace {ws} floats = {ws * 4 / 2 ** 20:.1f} MiB")
        for B in (36, 1):
            gen = torch.Generator().manual_seed(B)
            z = torch.randn(B, m.latent_dim, FRAMES, generator=gen).cuda()
            w = torch.randn(B, 1, m.output_samples(FRAMES), generator=gen).cuda()
            grads = {}

            def params():
                m.set_trainable("decoder")
                for p in dec.values():
                    p.grad = None
                zt = z.clone().requires_grad_(True)
                (m.decode(zt) * w).sum().backward()
                grads["params"] = {k: p.grad for k, p in dec.items()}

            def latent():
                m.set_trainable(None)
                zt = z.clone().requires_grad_(True)
                (m.decode(zt) * w).sum().backward()
                grads["latent"] = zt.grad

            def eager():
                for p in leaves.values():
                    p.grad = None
                zt = z.clone().requires_grad_(True)
                (ref.decoder(zt) * w).sum().backward()
                grads["eager"] = {k: p.grad for k, p in leaves.items()}

            fns = {"params": params, "latent": latent, "eager": eager}
            print(f"{name} {B} x 3 s ...", flush=True)
            mem ={arm: peak_above(fns[arm]) for arm in ARMS}
            diff = max(float((grads["params"][k] - grads["eager"][k]).norm() / grads["eager"][k].norm()) for k in dec)
            grads.clear()
            ms = {arm: [] for arm in ARMS}
            for _ in range(args.rounds):
                for arm in ARMS:
                    ms[arm].append(timed(fns[arm], args.steps, args.warmup))
            first = len(lines)
            lines.append(f"{name} {B:2d} x 3 s   worst tensor |g native - eager| / |eager| = {diff:.2e}")
            for arm in ARMS:
                v = ms[arm]
                lines.append(f"    {arm:6s} {np.median(v):9.2f} ms   rounds {' '.join(f'{x:.2f}' for x in v)}   spread {(max(v) - min(v)) / min(v) * 100:.1f} %   "
                             f"peak memory of one step {mem[arm]:.2f} GiB")
            med = {arm: float(np.median(ms[arm])) for arm in ARMS}
            lines.append(f"    eager / params = {med['eager'] / med['params']:.2f}   params - latent = {med['params'] - med['latent']:.2f} ms")
            print("\n".join(lines[first:]), flush=True)
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")
            grads.clear()
            for p in list(dec.values()) + list(leaves.values()):
                p.grad = None
            del z, w
            torch.cuda.empty_cache()
        m.set_trainable(None)
        del m, ref, leaves, dec
        torch.cuda.empty_cache()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
