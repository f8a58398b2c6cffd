"""The DAC baseline codec (esc.baselines.DAC) next to ESC-Base, in one process on one GPU: ms per call of encode, decode and eval forward for
DAC-Tiny and DAC-Base (16 kHz / 9 kbps configurations, name-keyed weights from esc.synth.dac_tensor) at 36 x 3 s and 1 x 3 s, ESC-Base at the
same batches (bench.py's model, all streams), and the torch-eager restatement (tests/dac_util.py) on the same GPU.  FLOPs are counted from the
convolution shapes (2 * MACs; the quantiser's projections and search are included in encode); TFLOP/s = FLOPs / time.  Host wall clock around
`--steps` synchronised calls, the same count for native and eager.  --snake-ab instead times native encode and decode for each Snake placement
(include/escx.h escx_dac_set_snake_maps: Snake on the staged operand, or a Snaked copy of the map, per layer class).  --precision-ab times native
encode / decode / forward in "fp32" and "bf16x3" (DAC.set_precision), the two modes alternating over --rounds rounds in one process with the same
warm-up and step counts; the spread of the fp32 rounds, (max - min) / min, is the noise a difference has to exceed.  ESC-Base's forward in
"bf16x3" is timed next to it for the like-for-like line.

    python tools/dac_timing.py [--steps 10] [--warmup 3] [--json OUT] [--snake-ab | --precision-ab [--rounds 3]]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import dac_util as du  # noqa: E402

CONFIGS = {
    "dac_tiny": dict(encoder_dim=32, encoder_rates=[2, 4, 5, 8], decoder_dim=288, decoder_rates=[8, 5, 4, 2], n_codebooks=18, codebook_size=1024,
                     codebook_dim=8, sample_rate=16000),
    "dac_base": dict(encoder_dim=64, encoder_rates=[2, 4, 5, 8], decoder_dim=1536, decoder_rates=[8, 5, 4, 2], n_codebooks=18, codebook_size=1024,
                     codebook_dim=8, sample_rate=16000),
}


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def flops(cfg, B, L):
    """(encode, decode) FLOPs of one batch from the layer shapes."""
    c = du.full_config(cfg)
    enc = 0
    t, ch = L, c["encoder_dim"]
    enc += 2 * B * t * ch * 7
    for s in c["encoder_rates"]:
        enc += 3 * 2 * B * t * ch * ch * (7 + 1)
        t = (t + 2 * math.ceil(s / 2) - 2 * s) // s + 1
        enc += 2 * B * t * (2 * ch) * ch * 2 * s
        ch *= 2
    D, d, K, n = c["latent_dim"], c["codebook_dim"], c["codebook_size"], c["n_codebooks"]
    enc += 2 * B * t * ch * D * 3 + n * 2 * B * t * (D * d + K * d + d * D)
    T = t
    dec = 2 * B * T * D * c["decoder_dim"] * 7
    ch = c["decoder_dim"]
    for s in c["decoder_rates"]:
        T = (T - 1) * s - 2 * math.ceil(s / 2) + 2 * s
        dec += 2 * B * T * ch * (ch // 2) * 2          # each output sample takes two taps of the transposed convolution
        ch //= 2
        dec += 3 * 2 * B * T * ch * ch * (7 + 1)
    dec += 2 * B * T * ch * 7
    return enc, dec


def dac_model(name, dev):
    from esc import synth
    from esc.baselines import DAC
    m = DAC(**CONFIGS[name])
    man = {k: list(v.shape) for k, v in m.state_dict().items()}
    m.load_state_dict({k: torch.from_numpy(v) for k, v in synth.dac_state_dict(man).items()}, strict=True)
    return m.to(dev).eval(), {k: v.detach().clone() for k, v in m.state_dict().items()}


SNAKE_CLASSES = {"none": 0, "res7": 1, "res1": 2, "down": 4, "up": 8, "last": 16, "all": 31}


def snake_ab(a, dev):
    """ms per native encode / decode for each Snake placement: 'none' = Snake on the staged operand everywhere, a class name = a Snaked map for
    that class only, 'all' = Snaked maps everywhere, 'default' = the library's default."""
    from esc import synth
    from esc import _native
    rows = []
    for name in CONFIGS:
        m, _ = dac_model(name, dev)
        default = _native.load().escx_dac_get_snake_maps(m._handle(dev)[1])
        for B in (36, 1):
            pcm = np.stack([synth.voiced_clip_int16(f"dac-time-{i}", 48000) if i % 2 else synth.noise_clip_int16(f"dac-time-{i}", 48000) for i in range(B)])
            x = torch.from_numpy(synth.pcm_to_float(pcm))[:, None].to(dev)
            for tag, mask in list(SNAKE_CLASSES.items()) + [("default", default)]:
                m.set_snake_maps(mask)
                z = m.encode(x)[0]
                r = {"model": name, "batch": B, "snake_maps": tag, "mask": mask,
                     "encode": round(timed(lambda: m.encode(x), a.steps, a.warmup), 3), "decode": round(timed(lambda: m.decode(z), a.steps, a.warmup), 3)}
                rows.append(r)
                print(json.dumps(r), flush=True)
        m.set_snake_maps(default)
        del m
        torch.cuda.empty_cache()
    return rows


def precision_ab(a, dev):
    """Per model and batch: ms per call of each mode (mean and every round), the fp32 run-to-run spread and fp32 / bf16x3."""
    from esc import synth
    rows = []
    ops = ("encode", "decode", "forward")
    for name in CONFIGS:
        m, _ = dac_model(name, dev)
        for B in (36, 1):
            pcm = np.stack([synth.voiced_clip_int16(f"dac-time-{i}", 48000) if i % 2 else synth.noise_clip_int16(f"dac-time-{i}", 48000) for i in range(B)])
            x = torch.from_numpy(synth.pcm_to_float(pcm))[:, None].to(dev)
            z = m.encode(x)[0]
            fns = {"encode": lambda: m.encode(x), "decode": lambda: m.decode(z), "forward": lambda: m(x)}
            t = {mode: {op: [] for op in ops} for mode in ("fp32", "bf16x3")}
            for _ in range(a.rounds):
                for mode in ("fp32", "bf16x3"):
                    m.set_precision(mode)
                    for op in ops:
                        t[mode][op].append(timed(fns[op], a.steps, a.warmup))
            m.set_precision("fp32")
            for op in ops:
                f, b = t["fp32"][op], t["bf16x3"][op]
                r = {"model": name, "batch": B, "op": op, "fp32_ms": round(sum(f) / len(f), 3), "bf16x3_ms": round(sum(b) / len(b), 3),
                     "fp32_rounds": [round(v, 3) for v in f], "bf16x3_rounds": [round(v, 3) for v in b],
                     "fp32_spread": round((max(f) - min(f)) / min(f), 4), "speedup": round(sum(f) / sum(b), 3)}
                rows.append(r)
                print(json.dumps(r), flush=True)
        del m
        torch.cuda.empty_cache()
    esc_model = bench.build_model(dev)[0]
    esc_model.set_precision("bf16x3")
    s = getattr(esc_model, "max_streams", 6)
    for B in (36, 1):
        xe = bench.synth_batch(B, 0).to(dev)
        f = [timed(lambda: esc_model(xe, None, s), a.steps, a.warmup) for _ in range(a.rounds)]
        r = {"model": "esc_base", "batch": B, "op": "forward", "bf16x3_ms": round(sum(f) / len(f), 3), "bf16x3_rounds": [round(v, 3) for v in f]}
        rows.append(r)
        print(json.dumps(r), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--json", default=None)
    ap.add_argument("--snake-ab", action="store_true")
    ap.add_argument("--precision-ab", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.snake_ab or a.precision_ab:
        rows = snake_ab(a, dev) if a.snake_ab else precision_ab(a, dev)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(rows, f, indent=1)
        return
    from esc import synth
    esc_model = bench.build_model(dev)[0]
    rows = []
    for B in (36, 1):
        pcm = np.stack([synth.voiced_clip_int16(f"dac-time-{i}", 48000) if i % 2 else synth.noise_clip_int16(f"dac-time-{i}", 48000) for i in range(B)])
        x = torch.from_numpy(synth.pcm_to_float(pcm))[:, None].to(dev)
        xe = bench.synth_batch(B, 0).to(dev)
        s = getattr(esc_model, "max_streams", 6)
        codes, shape = esc_model.encode(xe, s)
        r = {"model": "esc_base", "impl": "native", "batch": B,
             "encode": timed(lambda: esc_model.encode(xe, s), a.steps, a.warmup),
             "decode": timed(lambda: esc_model.decode(codes, shape), a.steps, a.warmup),
             "forward": timed(lambda: esc_model(xe, None, s), a.steps, a.warmup)}
        rows.append(r)
        print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
        for name in CONFIGS:
            m, sd = dac_model(name, dev)
            fe, fd = flops(CONFIGS[name], B, x.shape[-1])
            z = m.encode(x)[0]
            r = {"model": name, "impl": "native", "batch": B,
                 "encode": timed(lambda: m.encode(x), a.steps, a.warmup),
                 "decode": timed(lambda: m.decode(z), a.steps, a.warmup),
                 "forward": timed(lambda: m(x), a.steps, a.warmup), "gflop_encode": fe / 1e9, "gflop_decode": fd / 1e9}
            r["tflops_encode"], r["tflops_decode"] = fe / r["encode"] / 1e9, fd / r["decode"] / 1e9
            rows.append(r)
            print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
            ref = du.DacRef(CONFIGS[name], {k: v.to(dev) for k, v in sd.items()})
            with torch.no_grad():
                zr = ref.encode(x)[0]
                r = {"model": name, "impl": "torch_eager", "batch": B,
                     "encode": timed(lambda: ref.encode(x), a.steps, a.warmup),
                     "decode": timed(lambda: ref.decoder(zr), a.steps, a.warmup),
                     "forward": timed(lambda: ref.forward(x), a.steps, a.warmup)}
            rows.append(r)
            print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in r.items()}), flush=True)
            del m, ref
            torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
