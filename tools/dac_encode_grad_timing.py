"""Encode forward + backward and full forward + backward of the DAC baseline (esc.baselines.DAC.encode / forward with audio that requires grad:
include/escx.h escx_dac_encode_tape / escx_dac_encode_backward, then escx_dac_decode_tape / escx_dac_decode_backward) next to torch-eager autograd
of the restatement with the reference's detaches (tests/dac_encode_grad_util.DacRefE) on the same GPU, in one process:
    encode:   z, _, lat, cm, _ = encode(x); ((z * w_z).sum() + (lat * w_lat).sum() + cm * w_cm).backward()
    forward:  (forward(x)["audio"] * w).sum().backward()
in ms per step for DAC-Tiny and DAC-Base at 36 x 3 s and 1 x 3 s (16 kHz, 48000 samples, 150 frames).  The two arms alternate over --rounds
rounds with the same warm-up and step counts; every step ends in a device synchronise inside the host-clock window.  The spread,
(max - min) / min over an arm's rounds, is the noise a difference has to exceed.  Also printed: the encode tape's size
(escx_dac_encode_tape_floats), the peak of torch's device allocator during one step of each arm (the handle's scratch is its own allocation and
not in it), and the two arms' gradients against each other (the eager arm chooses its own codes; a row where they differ shows in that figure).

    python tools/dac_encode_grad_timing.py [--steps 3] [--warmup 1] [--rounds 3] [--out profiles/dac_encode_grad_timing.txt]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dac_encode_grad_util as eu  # noqa: E402
from dac_grad_timing import CONFIGS, peak_above, timed  # noqa: E402
from esc import synth  # noqa: E402

SAMPLES = 48000     # 3 s at 16 kHz: 150 frames at hop 320


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dac_encode_grad_timing.txt"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is no fallback"
    from esc.baselines import DAC
    lines = [f"encode / forward with their backward, ms per step (host clock around {args.steps} synchronised steps, {args.warmup} warm-up, {args.rounds} alternating rounds)",
             f"device: {torch.cuda.get_device_name(0)}   torch {torch.__version__}", ""]
    for name, cfg in CONFIGS.items():
        m = DAC(**cfg)
        sd = {k: torch.from_numpy(synth.dac_tensor(k, tuple(v.shape))) for k, v in m.state_dict().items()}
        m.load_state_dict(sd, strict=True)
        m = m.cuda().eval()
        ref = eu.DacRefE(cfg, {k: v.cuda() for k, v in sd.items()}, torch.float32)
        lib, hd = m._handle(torch.device("cuda:0"))
        n, d = m.n_codebooks, m.codebook_dim
        for B in (36, 1):
            gen = torch.Generator().manual_seed(B)
            T = m.num_frames(SAMPLES)
            x = (0.5 * torch.randn(B, 1, SAMPLES, generator=gen)).cuda()
            w_z, w_lat = torch.randn(B, m.latent_dim, T, generator=gen).cuda(), torch.randn(B, n * d, T, generator=gen).cuda()
            w_cm, w = float(d * T), torch.randn(B, 1, SAMPLES, generator=gen).cuda()
            grads = {}

            def enc_native():
                xt = x.clone().requires_grad_(True)
                z, _, lat, cm, _ = m.encode(xt)
                ((z * w_z).sum() + (lat * w_lat).sum() + cm * w_cm).backward()
                grads["enc native"] = xt.grad

            def enc_eager():
                xt = x.clone().requires_grad_(True)
                o = ref.encode_dict(xt)
                ((o["z"] * w_z).sum() + (o["latents"] * w_lat).sum() + o["cm"] * w_cm).backward()
                grads["enc eager"] = xt.grad

            def fwd_native():
                xt = x.clone().requires_grad_(True)
                a = m(xt)["audio"]                          # 320 T - 8 samples: shorter than the input, as the reference's
                (a * w[..., :a.shape[-1]]).sum().backward()
                grads["fwd native"] = xt.grad

            def fwd_eager():
                xt = x.clone().requires_grad_(True)
                a = ref.forward_dict(xt)["audio"]
                (a * w[..., :a.shape[-1]]).sum().backward()
                grads["fwd eager"] = xt.grad

            tape = int(lib.escx_dac_encode_tape_floats(hd, B, SAMPLES, n))
            lines.append(f"{name} {B:2d} x 3 s   encode tape {tape} floats = {tape * 4 / 2 ** 30:.3f} GiB")
            for what, native, eager in (("encode ", enc_native, enc_eager), ("forward", fwd_native, fwd_eager)):
                k = what.strip()[:3]
                mem = {"native": peak_above(native), "eager": peak_above(eager)}
                diff = float((grads[k + " native"] - grads[k + " eager"]).norm() / grads[k + " eager"].norm())
                ms = {"native": [], "eager": []}
                for _ in range(args.rounds):
                    for arm, fn in (("native", native), ("eager", eager)):
                        ms[arm].append(timed(fn, args.steps, args.warmup))
                lines.append(f"  {what} + backward   |d_x native - eager| / |eager| = {diff:.2e}")
                for arm in ("native", "eager"):
                    v = ms[arm]
                    lines.append(f"    {arm:6s} {np.median(v):9.2f} ms   rounds {' '.join(f'{t:.2f}' for t in v)}   spread {(max(v) - min(v)) / min(v) * 100:.1f} %   "
                                 f"peak memory of one step {mem[arm]:.2f} GiB")
                lines.append(f"    eager / native = {np.median(ms['eager']) / np.median(ms['native']):.2f}")
                grads.clear()
                torch.cuda.empty_cache()
            print("\n".join(lines[-11:]), flush=True)
            del x, w_z, w_lat, w
            torch.cuda.empty_cache()
        del m, ref
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
