"""DAC's chunked compress / decompress (esc.baselines.DAC.compress): the reference's schedule, one window per pass (chunks_per_pass = 1), against
every window of the file as one batch (the default), in one process on one GPU.  DAC-Base and DAC-Tiny (16 kHz / 9 kbps configurations,
name-keyed weights) on a 60 s synthetic signal at win_duration = 1.0: ms per compress and per decompress of the whole file.  The two arms
alternate over --rounds rounds with the same warm-up and step counts; the spread of the sequential rounds, (max - min) / min, is the noise a
difference has to exceed.  Both arms produce the same codes and the same audio, asserted before timing.

    python tools/dac_chunk_timing.py [--seconds 60] [--steps 3] [--warmup 1] [--rounds 3] [--json OUT] > profiles/dac_chunk_timing.txt
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

import dac_timing as dt  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--win_duration", type=float, default=1.0)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--models", default="dac_tiny,dac_base")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from esc import synth
    dev = torch.device("cuda:0")
    nt = int(a.seconds * 16000)
    pcm = np.concatenate([synth.voiced_clip_int16(f"dac-chunk-time-{i}", 48000) if i % 2 else synth.noise_clip_int16(f"dac-chunk-time-{i}", 48000)
                          for i in range(-(-nt // 48000))])[:nt]
    x = torch.from_numpy(synth.pcm_to_float(pcm))[None, None].to(dev)
    rows = []
    print(f"# python tools/dac_chunk_timing.py --seconds {a.seconds} --win_duration {a.win_duration} --steps {a.steps} --warmup {a.warmup} --rounds {a.rounds}"
          f"   (MI355X, one process, ms per whole-file call on {nt} samples; seq_spread = (max - min) / min of the chunks_per_pass = 1 rounds)", flush=True)
    for name in a.models.split(","):
        m = dt.dac_model(name, dev)[0]
        sch = m.chunk_schedule(nt, a.win_duration)
        f1 = m.compress(x, win_duration=a.win_duration, chunks_per_pass=1)
        f = m.compress(x, win_duration=a.win_duration)
        assert torch.equal(f.codes, f1.codes) and torch.equal(m.decompress(f), m.decompress(f, chunks_per_pass=1)), name
        fns = {"compress": (lambda: m.compress(x, win_duration=a.win_duration, chunks_per_pass=1), lambda: m.compress(x, win_duration=a.win_duration)),
               "decompress": (lambda: m.decompress(f, chunks_per_pass=1), lambda: m.decompress(f))}
        for op, (seq_fn, one_fn) in fns.items():
            seq, one = [], []
            for _ in range(a.rounds):
                seq.append(dt.timed(seq_fn, a.steps, a.warmup))
                one.append(dt.timed(one_fn, a.steps, a.warmup))
            spread = (max(seq) - min(seq)) / min(seq)
            ms_s, ms_o = sum(seq) / len(seq), sum(one) / len(one)
            r = {"model": name, "op": op, "precision": m.precision, "chunks": len(sch["starts"]), "n_samples": sch["n_samples"], "hop": sch["hop"],
                 "chunk_length": sch["chunk_length"], "per_chunk_passes_ms": round(ms_s, 3), "one_batch_ms": round(ms_o, 3),
                 "per_chunk_rounds": [round(v, 3) for v in seq], "one_batch_rounds": [round(v, 3) for v in one], "seq_spread": round(spread, 4),
                 "speedup": round(ms_s / ms_o, 3), "faster_beyond_spread": bool(ms_s / ms_o - 1.0 > spread)}
            rows.append(r)
            print(json.dumps(r), flush=True)
        del m
        torch.cuda.empty_cache()
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
