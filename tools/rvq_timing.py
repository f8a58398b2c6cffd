"""The rvq+swinT codec (RVQCodecs) next to ESC-Base on the bench's 36 clips of 3 s, in the same process: ms per call of encode, decode and
eval forward at S = 1..6, in the default precision and in bf16x3 (host wall clock around `--steps` synchronised calls, as
tools/mixed_streams_timing.py).  Both models carry name-keyed synthetic weights (esc/synth.py); rvq+swinT uses the ablation yaml's
configuration (tests/golden/rvq_base.npz).  --profile adds the per-kernel report of one rvq encode and one rvq forward at S = 6 with the
quantiser kernel's share of the kernel time.

    python tools/rvq_timing.py [--steps 30] [--warmup 5] [--profile]
"""
import argparse
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


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def rvq_model(dev):
    from esc import synth
    from esc.models import make_model
    g = np.load(os.path.join(ROOT, "tests", "golden", "rvq_base.npz"))
    model = make_model(json.loads(str(g["config_json"])), "rvq+swinT")
    sd = {}
    for k, shp in model._state_manifest().items():
        v = torch.hann_window(shp[0]).numpy() if k.endswith(".window") else synth.synth_tensor(k, shp)
        sd[k] = torch.from_numpy(np.ascontiguousarray(v))
    model.load_state_dict(sd, strict=True)
    return model.to(dev).eval()


def profile(model, dev, fn):
    lib, hd = model._handle(dev)
    lib.escx_profile_enable(hd, 1)
    fn()
    torch.cuda.synchronize()
    rep = json.loads(lib.escx_profile_report(hd).decode())
    lib.escx_profile_enable(hd, 0)
    tot = sum(r["ms"] for r in rep)
    q = sum(r["ms"] for r in rep if r["name"].startswith("prvq"))
    return {"kernel_ms": round(tot, 3), "prvq_ms": round(q, 4), "prvq_share": round(q / tot, 4) if tot else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    models = {"rvq+swinT": rvq_model(dev), "esc_base": bench.build_model(dev)[0]}
    x = bench.synth_batch(36, 0).to(dev)
    rows = []
    for mode in (models["esc_base"].precision, "bf16x3"):
        for name, model in models.items():
            model.set_precision(mode)
            for s in range(1, 7):
                codes, shape = model.encode(x, s)
                r = {"model": name, "precision": mode, "S": s,
                     "encode": round(timed(lambda: model.encode(x, s), a.steps, a.warmup), 3),
                     "decode": round(timed(lambda: model.decode(codes, shape), a.steps, a.warmup), 3),
                     "forward": round(timed(lambda: model(x, None, s), a.steps, a.warmup), 3)}
                print(f"{mode:7s} {name:10s} S={s}  encode {r['encode']:7.3f}  decode {r['decode']:7.3f}  forward {r['forward']:7.3f} ms", flush=True)
                rows.append(r)
        if a.profile:
            m = models["rvq+swinT"]
            for what, fn in (("encode", lambda: m.encode(x, 6)), ("forward", lambda: m(x, None, 6))):
                p = profile(m, dev, fn)
                print(f"{mode:7s} rvq+swinT {what} S=6 kernels {p['kernel_ms']:.3f} ms, quantiser {p['prvq_ms']:.4f} ms ({100 * p['prvq_share']:.2f} %)",
                      flush=True)
                rows.append(dict(p, model="rvq+swinT", precision=mode, profile=what))
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
