"""A/B of the DAC baseline's backward arithmetic (esc.baselines.DAC.set_grad_precision, include/escx.h escx_dac_set_grad_precision): grad mode fp32
against bf16x3 in one process, ms per step of forward + backward, for the three differentiable paths

    decoder dX   audio = decode(z), z requires grad                       escx_dac_decode_tape / escx_dac_decode_backward
    encoder dX   z, _, latents, cm, _ = encode(x), x requires grad        escx_dac_encode_tape / escx_dac_encode_backward
    params       decode(z) after set_trainable("decoder")                 escx_dac_decode_backward_params (dX under the mode, dW on the fp32 MFMA)

for DAC-Base and DAC-Tiny at 36 x 3 s and 1 x 3 s (16 kHz), with the forward in fp32 and in bf16x3.  The forward is the same code in both arms, so
the difference of two arms is the backward's.  The arms alternate over --rounds rounds; every timed window is at least --window-ms of
synchronised steps after a warm-up of the same shape.  The spread, (max - min) / min over the fp32 arm's rounds, is the noise a difference has
to exceed.  Also printed: the two arms' gradients against each other at the timed size.

    python tools/dac_grad_precision_ab.py [--rounds 3] [--window-ms 500] [--out profiles/dac_grad_precision_ab.txt]
"""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from esc import synth  # noqa: E402

CONFIGS = {
    "dac_base": dict(encoder_dim=64, encoder_rates=[2, 4, 5, 8], decoder_dim=1536, decoder_rates=[8, 5, 4, 2], n_codebooks=18, codebook_size=1024,
                     codebook_dim=8, sample_rate=16000),
    "dac_tiny": dict(encoder_dim=32, encoder_rates=[2, 4, 5, 8], decoder_dim=288, decoder_rates=[8, 5, 4, 2], n_codebooks=18, codebook_size=1024,
                     codebook_dim=8, sample_rate=16000),
}
FRAMES = 150        # 3 s at 16 kHz, hop 320
ARMS = ("fp32", "bf16x3")


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
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--window-ms", type=float, default=500.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dac_grad_precision_ab.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no fallback"
    from esc.baselines import DAC
    lines = [f"forward + backward, ms per step: grad mode fp32 against bf16x3 (host clock around >= {args.window_ms:.0f} ms of synchronised steps, "
             f"{args.warmup} warm-up, {args.rounds} alternating rounds)",
             f"device: {torch.cuda.get_device_name(0)}   torch {torch.__version__}",
             "spread = (max - min) / min over the fp32 arm's rounds; gain = median fp32 / median bf16x3", ""]
    for name, cfg in CONFIGS.items():
        m = DAC(**cfg)
        sd = {k: torch.from_numpy(synth.dac_tensor(k, tuple(v.shape))) for k, v in m.state_dict().items()}
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval()
        for B in (36, 1):
            gen = torch.Generator().manual_seed(B)
            z = torch.randn(B, m.latent_dim, FRAMES, generator=gen).cuda()
            L = m.output_samples(FRAMES)
            w = torch.randn(B, 1, L, generator=gen).cuda()
            x = torch.rand(B, 1, L, generator=gen).sub_(0.5).cuda()
            wz = torch.randn(B, m.latent_dim, FRAMES, generator=gen).cuda()
            out = {}

            def decoder_dx():
                zt = z.clone().requires_grad_(True)
                (m.decode(zt) * w).sum().backward()
                out["g"] = zt.grad

            def encoder_dx():
                xt = x.clone().requires_grad_(True)
                (m.encode(xt)[0] * wz).sum().backward()
                out["g"] = xt.grad

            def params():
                for p in m.decoder_parameters():
                    p.grad = None
                zt = z.clone().requires_grad_(True)
                (m.decode(zt) * w).sum().backward()
                out["g"] = torch.cat([p.grad.reshape(-1) for p in m.decoder_parameters()])

            for part, fn in (("decoder dX", decoder_dx), ("encoder dX", encoder_dx), ("params", params)):
                trainable = part == "params"
                m.set_trainable("decoder" if trainable else None)
                for k, p in m.named_parameters():
                    p.requires_grad_(trainable and k.startswith("decoder."))
                    p.grad = None
                for fwd in ARMS:
                    m.set_precision(fwd)
                    g = {}
                    for arm in ARMS:                            # first run of each arm: allocations, mirrors, and the gradients to compare
                        m.set_grad_precision(arm)
                        fn()
                        torch.cuda.synchronize()
                        g[arm] = out["g"].clone()
                    diff = float((g["bf16x3"] - g["fp32"]).norm() / g["fp32"].norm())
                    steps = max(2, math.ceil(args.window_ms / timed(fn, 2, 1)))
                    ms = {arm: [] for arm in ARMS}
                    for _ in range(args.rounds):
                        for arm in ARMS:
                            m.set_grad_precision(arm)
                            ms[arm].append(timed(fn, steps, args.warmup))
                    med = {arm: float(np.median(ms[arm])) for arm in ARMS}
                    spread = (max(ms["fp32"]) - min(ms["fp32"])) / min(ms["fp32"])
                    lines.append(f"{name} {B:2d} x 3 s  {part:10s} forward {fwd:6s}  fp32 {med['fp32']:8.2f}  bf16x3 {med['bf16x3']:8.2f}  gain {med['fp32'] / med['bf16x3']:.3f}  "
                                 f"fp32 spread {spread * 100:.1f} %  ({steps} steps)  rounds fp32 {' '.join(f'{v:.2f}' for v in ms['fp32'])} | bf16x3 "
                                 f"{' '.join(f'{v:.2f}' for v in ms['bf16x3'])}  |g bf16x3 - g fp32| / |g fp32| = {diff:.2e}")
                    print(lines[-1], flush=True)
                    g.clear()
            m.set_precision("fp32").set_grad_precision("fp32").set_trainable(None)
            out.clear()
            del z, w, x, wz
            torch.cuda.empty_cache()
        del m
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
