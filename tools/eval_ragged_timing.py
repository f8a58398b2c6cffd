"""What one evaluation step over a test set of whole utterances costs (scripts/test.py --ragged), in one process on one GPU.  36 synthetic clips with
the fixed-seed lengths of tools/esc_lengths_timing.py (0.5 s to 3 s at 16 kHz), each snapped to the longest length the model reconstructs in full
(scripts.utils.snap_length), ESC-Base and DAC-Tiny (name-keyed weights), one bitrate.  A step is the forward, the mel distance, SI-SDR and the
code-utilisation update, with the per-clip values fetched to the host as eval_epoch does.  Three arms alternate over --rounds rounds, each timed over a
window of at least --window seconds after a warm-up:
  ragged_native    one `lengths` call on the zero-padded batch + the length-aware HIP metrics of esc.metrics
  ragged_scripts   the same call + the plain-torch scripts.metrics classes applied clip by clip on x[b, :L_b]
  per_clip         the batch-size-1 loop with the scripts.metrics classes (the reference's way)
ms per step; <arm>_spread = (max - min) / min of that arm's rounds is the noise a difference between arms has to exceed.  The two `metrics_*` figures
time the metric half alone on the ragged call's outputs (native batch against scripts clip by clip).  Before timing, the native arm's per-clip
values are compared with the scripts arm's.

    python tools/eval_ragged_timing.py [--clips 36] [--rounds 3] [--window 0.5] [--json OUT] > profiles/eval_ragged_timing.txt
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from esc_lengths_timing import window_ms  # noqa: E402


def load(name, dev):
    """(model behind eval_epoch's interface, num_streams of the timed bitrate, (codebook_size, code slots, groups))."""
    from scripts.test import DacEvalModel
    if name.startswith("dac_"):
        import dac_timing as dt
        m = DacEvalModel(dt.dac_model(name, dev)[0]).eval()
        s = m.max_streams
        return m, s, (m.dac.codebook_size, m.code_slots(s), 1)
    from gpu_util import build_models
    m, _, _, cfg = build_models(name)
    return m, cfg["max_streams"], (cfg["codebook_size"], cfg["max_streams"], cfg["group_size"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=36)
    ap.add_argument("--min_seconds", type=float, default=0.5)
    ap.add_argument("--max_seconds", type=float, default=3.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--models", default="base,dac_tiny")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    from esc import metrics as NM
    from esc import synth
    from scripts import metrics as M
    from scripts.utils import snap_length
    dev = torch.device("cuda:0")
    sr = 16000
    drawn = np.random.RandomState(a.seed).randint(int(a.min_seconds * sr), int(a.max_seconds * sr) + 1, size=a.clips).tolist()
    rows = []
    print(f"# python tools/eval_ragged_timing.py --clips {a.clips} --min_seconds {a.min_seconds} --max_seconds {a.max_seconds} --seed {a.seed} --rounds {a.rounds} "
          f"--warmup {a.warmup} --window {a.window} --models {a.models}   (MI355X, one process, ms per evaluation step of {a.clips} clips at one bitrate; "
          f"<arm>_spread = (max - min) / min of the arm's rounds)", flush=True)
    for name in a.models.split(","):
        model, S, (K, slots, G) = load(name, dev)
        lens = sorted((snap_length(model, n) for n in drawn), reverse=True)                  # the harness forms batches longest first
        Lmax = lens[0]
        pcm = np.zeros((a.clips, Lmax), np.int16)
        for i, n in enumerate(lens):
            pcm[i, :n] = (synth.voiced_clip_int16 if i % 2 else synth.noise_clip_int16)(f"eval-ragged-time-{i}", Lmax)[:n]
        x = torch.from_numpy(synth.pcm_to_float(pcm)).to(dev)
        clips = [x[b:b + 1, :n].contiguous() for b, n in enumerate(lens)]
        n_mel, n_sdr, n_ec = NM.MelSpectrogramDistance().to(dev), NM.SISDR().to(dev), NM.EntropyCounter(K, slots, G, dev)
        s_mel, s_sdr, s_ec = M.MelSpectrogramDistance().to(dev), M.SISDR().to(dev), M.EntropyCounter(K, slots, G, dev)
        fwd = lambda t, **k: model(**dict(x=t, x_feat=None, num_streams=S, **k))            # noqa: E731

        def native_metrics(out):
            vals = n_mel(x, out["recon_audio"], lengths=lens).tolist(), n_sdr(x, out["recon_audio"], lengths=lens).tolist()
            n_ec.update(out["codes"])
            return vals

        def scripts_metrics(out):
            mel, sdr = [], []
            for b, n in enumerate(lens):
                r = out["recon_audio"][b:b + 1, :n]
                mel += s_mel(clips[b], r).tolist(); sdr += s_sdr(clips[b], r).tolist()
                c = out["codes"][b:b + 1]
                s_ec.update(c[..., :int((c[0, 0, 0] >= 0).sum())])
            return mel, sdr

        def per_clip():
            mel, sdr = [], []
            for c in clips:
                out = fwd(c)
                mel += s_mel(c, out["recon_audio"]).tolist(); sdr += s_sdr(c, out["recon_audio"]).tolist()
                s_ec.update(out["codes"])
            return mel, sdr

        with torch.no_grad():
            out = fwd(x, lengths=lens)
            nv, sv = native_metrics(out), scripts_metrics(out)
            mel_diff = float(np.max(np.abs(np.array(nv[0]) - np.array(sv[0]))))
            sdr_diff = float(np.max(np.abs(np.array(nv[1]) - np.array(sv[1]))))
            util_equal = n_ec.compute_utilization() == s_ec.compute_utilization()
            arms = {"ragged_native": lambda: native_metrics(fwd(x, lengths=lens)), "ragged_scripts": lambda: scripts_metrics(fwd(x, lengths=lens)),
                    "per_clip": per_clip, "metrics_native": lambda: native_metrics(out), "metrics_scripts": lambda: scripts_metrics(out)}
            t = {k: [] for k in arms}
            for _ in range(a.rounds):
                for arm, fn in arms.items():
                    n_ec.reset_stats(slots); s_ec.reset_stats(slots)
                    t[arm].append(window_ms(fn, a.warmup, a.window))
        mean = {k: sum(v) / len(v) for k, v in t.items()}
        r = {"model": name, "num_streams": S, "clips": a.clips, "live_fraction": round(sum(lens) / (a.clips * Lmax), 4),
             "max_abs_mel_difference_native_vs_scripts": mel_diff, "max_abs_sisdr_difference_native_vs_scripts": sdr_diff, "utilization_equal": bool(util_equal)}
        for k, v in t.items():
            r[k + "_ms"] = round(mean[k], 3); r[k + "_rounds"] = [round(u, 3) for u in v]; r[k + "_spread"] = round((max(v) - min(v)) / min(v), 4)
        r["ragged_native_over_per_clip"] = round(mean["ragged_native"] / mean["per_clip"], 4)
        r["ragged_native_over_ragged_scripts"] = round(mean["ragged_native"] / mean["ragged_scripts"], 4)
        r["metrics_native_over_metrics_scripts"] = round(mean["metrics_native"] / mean["metrics_scripts"], 4)
        rows.append(r)
        print(json.dumps(r), flush=True)
        del model
        torch.cuda.empty_cache()
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
