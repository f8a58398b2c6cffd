"""The evaluation sweep of scripts/test.py, sequential (eval_epoch: the whole eval forward once per bitrate) against one-pass
(eval_epoch_one_pass: one encode per batch, one decode per bitrate), in one process on one GPU: ms per evaluation batch of 36 x 3 s over six
bitrates for ESC-Base (bench.py's model), DAC-Tiny and DAC-Base (16 kHz / 9 kbps configurations, name-keyed weights), each in its default
precision.  What is timed is the harness's own model work for one batch - the six `model(x=x, x_feat=None, num_streams=s)` calls of
_bitrate_pass, and `_sweep(model, x, [1..6])` - without the metrics, which are the same work in both arms.  The clips are as EvalSet serves
them (3 s minus the last 80 samples).  The two arms alternate over --rounds rounds with the same warm-up and step counts; the spread of the
sequential rounds, (max - min) / min, is the noise a difference has to exceed.

    python tools/eval_sweep_timing.py [--steps 5] [--warmup 2] [--rounds 3] [--json OUT]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import dac_timing as dt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batch", type=int, default=36)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from esc import synth
    from scripts.test import DacEvalModel, _sweep
    dev = torch.device("cuda:0")
    pcm = np.stack([synth.voiced_clip_int16(f"dac-time-{i}", 48000) if i % 2 else synth.noise_clip_int16(f"dac-time-{i}", 48000) for i in range(a.batch)])
    x = torch.from_numpy(synth.pcm_to_float(pcm))[:, :-80].to(dev)
    rows = []
    print(f"# python tools/eval_sweep_timing.py --steps {a.steps} --warmup {a.warmup} --rounds {a.rounds}   (MI355X, one process, ms per evaluation batch of "
          f"{a.batch} x {x.shape[-1]} samples over six bitrates; seq_spread = (max - min) / min of the sequential rounds)", flush=True)
    for name in ("esc_base", "dac_tiny", "dac_base"):
        if name == "esc_base":
            model = bench.build_model(dev)[0].eval()
        else:
            model = DacEvalModel(dt.dac_model(name, dev)[0]).eval()
        streams = list(range(1, model.max_streams + 1))
        assert len(streams) == 6
        with torch.no_grad():
            seq_fn = lambda: [model(x=x, x_feat=None, num_streams=s) for s in streams]          # noqa: E731
            one_fn = lambda: _sweep(model, x, streams)                                          # noqa: E731
            for o, (recon, codes) in zip(seq_fn(), one_fn()):                                   # the arms compute the same tensors
                assert torch.equal(o["recon_audio"], recon) and torch.equal(o["codes"], codes), name
            seq, one = [], []
            for _ in range(a.rounds):
                seq.append(dt.timed(seq_fn, a.steps, a.warmup))
                one.append(dt.timed(one_fn, a.steps, a.warmup))
        spread = (max(seq) - min(seq)) / min(seq)
        ms_s, ms_o = sum(seq) / len(seq), sum(one) / len(one)
        r = {"model": name, "batch": a.batch, "precision": getattr(model, "dac", model).precision, "sequential_ms": round(ms_s, 3), "one_pass_ms": round(ms_o, 3),
             "sequential_rounds": [round(v, 3) for v in seq], "one_pass_rounds": [round(v, 3) for v in one], "seq_spread": round(spread, 4),
             "speedup": round(ms_s / ms_o, 3), "faster_beyond_spread": bool(ms_s / ms_o - 1.0 > spread)}
        rows.append(r)
        print(json.dumps(r), flush=True)
        del model
        torch.cuda.empty_cache()
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
