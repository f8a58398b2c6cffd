"""A/B of the DAC baseline's weight-gradient arithmetic (esc.baselines.DAC.set_param_grad_precision, include/escx.h
escx_dac_set_param_grad_precision): param-grad mode fp32 (gemm_dw_kernel, 48 x 48 tiles on the fp32 MFMA) against bf16x3
(gemm_dw_bf16_kernel<DacConvA, DacConvA, 3>, 128 x 128 tiles, three bf16 terms per operand) in one process, ms per step of

    decode(z) forward + backward with every decoder parameter's gradient and d_z          escx_dac_decode_tape / escx_dac_decode_backward_params

for DAC-Base and DAC-Tiny at 36 x 3 s and 1 x 3 s (16 kHz), once with the forward and the input gradients in fp32 and once with both in bf16x3.
The forward and the input gradients are the same code in both arms, so the difference of two arms is the dW contractions'.  The arms alternate
over --rounds rounds; every timed window is at least --window-ms of synchronised steps after a warm-up of the same shape.  The spread,
(max - min) / min over the fp32 arm's rounds, is the noise a difference has to exceed.  Also printed: the two arms' parameter gradients against
each other at the timed size, and the handle's workspace in both modes.

    python tools/dac_param_grad_precision_ab.py [--rounds 3] [--window-ms 500] [--out profiles/dac_param_grad_precision_ab.txt]
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
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dac_param_grad_precision_ab.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no fallback"
    from esc.baselines import DAC
    lines = [f"decode forward + backward with parameter gradients, ms per step: param-grad mode fp32 against bf16x3 (host clock around >= "
             f"{args.window_ms:.0f} ms of synchronised steps, {args.warmup} warm-up, {args.rounds} alternating rounds)",
             f"device: {torch.cuda.get_device_name(0)}   torch {torch.__version__}",
             "spread = (max - min) / min over the fp32 arm's rounds; gain = median fp32 / median bf16x3", ""]
    for name in args.configs.split(","):
        m = DAC(**CONFIGS[name])
        sd = {k: torch.from_numpy(synth.dac_tensor(k, tuple(v.shape))) for k, v in m.state_dict().items()}
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval().set_trainable("decoder")
        for k, p in m.named_parameters():
            p.requires_grad_(k.startswith("decoder."))
        for B in (36, 1):
            gen = torch.Generator().manual_seed(B)
            z = torch.randn(B, m.latent_dim, FRAMES, generator=gen).cuda()
            w = torch.randn(B, 1, m.output_samples(FRAMES), generator=gen).cuda()
            out = {}

            def step():
                for p in m.decoder_parameters():
                    p.grad = None
                zt = z.clone().requires_grad_(True)
                (m.decode(zt) * w).sum().backward()
                out["g"] = torch.cat([p.grad.reshape(-1) for p in m.decoder_parameters()])

            for rest in ARMS:                                   # the forward's and the input gradients' mode, the same in both arms
                m.set_precision(rest).set_grad_precision(rest)
                g = {}
                for arm in ARMS:                                # first run of each arm: allocations, mirrors, and the gradients to compare
                    m.set_param_grad_precision(arm)
                    step()
                    torch.cuda.synchronize()
                    g[arm] = out["g"].clone()
                diff = float((g["bf16x3"] - g["fp32"]).norm() / g["fp32"].norm())
                steps = max(2, math.ceil(args.window_ms / timed(step, 2, 1)))
                ms = {arm: [] for arm in ARMS}
                for _ in range(args.rounds):
                    for arm in ARMS:
                        m.set_param_grad_precision(arm)
                        ms[arm].append(timed(step, steps, args.warmup))
                med = {arm: float(np.median(ms[arm])) for arm in ARMS}
                spread = (max(ms["fp32"]) - min(ms["fp32"])) / min(ms["fp32"])
                lines.append(f"{name} {B:2d} x 3 s  forward / grad {rest:6s}  fp32 {med['fp32']:8.2f}  bf16x3 {med['bf16x3']:8.2f}  gain {med['fp32'] / med['bf16x3']:.3f}  "
                             f"fp32 spread {spread * 100:.1f} %  ({steps} steps)  rounds fp32 {' '.join(f'{v:.2f}' for v in ms['fp32'])} | bf16x3 "
                             f"{' '.join(f'{v:.2f}' for v in ms['bf16x3'])}  |g bf16x3 - g fp32| / |g fp32| = {diff:.2e}")
                print(lines[-1], flush=True)
                g.clear()
            out.clear()
            del z, w
            torch.cuda.empty_cache()
        lib, hd, _, _, _ = m._ctx(torch.zeros(1, device="cuda"), "z")
        ws = {}
        for arm in ARMS:
            m.set_param_grad_precision(arm)
            ws[arm] = int(lib.escx_dac_param_grad_workspace_floats(hd))
        n_layers = 2 + 7 * len(m.decoder_rates)
        sl = {}
        for arm in ARMS:
            m.set_param_grad_precision(arm)
            sl[arm] = [int(lib.escx_dac_param_grad_slices(hd, 36, FRAMES, i)) for i in range(n_layers)]
        lines.append(f"{name} workspace, MB: fp32 {ws['fp32'] * 4 / 1e6:.1f}  bf16x3 {ws['bf16x3'] * 4 / 1e6:.1f} (the fp32 plan plus the 128 x 128 tiles' partial region)")
        lines.append(f"{name} slices per decoder layer at 36 x 3 s: fp32 {sl['fp32']}  bf16x3 {sl['bf16x3']}")
        lines.append("")
        print("\n".join(lines[-3:]), flush=True)
        m.set_precision("fp32").set_grad_precision("fp32").set_param_grad_precision("fp32")
        del m
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
