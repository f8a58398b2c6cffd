"""TEST INFRASTRUCTURE -- the DAC arm of the evaluation harness (scripts/test.py DacEvalModel): generates tests/golden/dac_eval.npz by running
the REAL reference DAC (baselines/descript of the reference repository, loaded as tools/gen_dac_golden.py loads it) on the CPU with the
dac_tiny configuration and name-keyed weights, and the reference's own metric classes (scripts/metrics.py of the reference on the shims of
oracle/ref_shims.py, as oracle/gen_metrics_golden.py uses them).  Run in the build container only:

    python tools/gen_dac_eval_golden.py [REFERENCE_ROOT]

Four 1 s clips, two noise and two voiced, in two batches of two, each without its last 80 samples, as the harness's EvalSet serves them
(scripts/utils.py:40 of the reference): 15920 samples, padded by DAC.forward to 50 frames and trimmed back.  Per kind the candidates are
ranked by their smallest reference argmin margin over every (frame, codebook) and the two largest are kept (the rule of tools/gen_rvq_golden.py::pick); the generator asserts that the kept
clips' smallest margin is at least 1e-5, five times the project's near-tie threshold of 2e-6, and widens the candidate set until it is, so that
the device's codes - and with them the utilisation - are the reference's exactly.  The fixture holds the PCM, the codes at 18 codebooks and the
per-bitrate table (utilisation, SI-SDR, mel distance; means rounded to 4 places as the reference's eval_epoch rounds them) at 3, 6, ..., 18
codebooks.  Data only; no reference source is stored.
"""
import importlib
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_dac_golden as gdg  # noqa: E402  (puts the product package and tests/ on sys.path; synth and dac_util come from there)
import ref_shims  # noqa: E402

NAME = "dac_tiny"
N_SAMPLES = 16000
NS = (3, 6, 9, 12, 15, 18)
MIN_MARGIN = 1e-5
KINDS = ("noise", "voiced")


def reference_metrics(ref_root):
    """The reference's scripts/metrics.py (torchaudio from the shim, pesq stubbed: PESQ is not part of the fixture)."""
    ref_shims.REFERENCE_ROOT = ref_root
    ref_shims.install()
    sys.modules["pesq"] = types.SimpleNamespace(pesq=lambda *a, **k: 0.0)
    for m in [m for m in sys.modules if m == "scripts" or m.startswith("scripts.")]:
        del sys.modules[m]
    return importlib.import_module("scripts.metrics")


def clip(kind, tag):
    return (gdg.synth.noise_clip_int16 if kind == "noise" else gdg.synth.voiced_clip_int16)(tag, N_SAMPLES)


def min_margin(model, ref, pcm):
    """Smallest second-best minus best distance of the reference's search over every frame and codebook of one clip, on the input the sweep
    encodes: the last 80 samples dropped, then DAC.preprocess's right padding."""
    x = torch.from_numpy(gdg.synth.pcm_to_float(pcm[None]))[:, None, :-80]
    with torch.no_grad():
        x = model.preprocess(x, None)
        codes = model.encode(x, None)[1]
        _, rcodes, _, _, _, mg = ref.quantize(model.encoder(x), None, margins=True)
    assert torch.equal(rcodes, codes), "restatement codes differ from the reference"
    return float(mg.min())


def pick(model, ref, per_kind=2, tries=6, max_tries=48):
    """Per kind the `per_kind` candidates with the largest smallest margin; more candidate tags are tried until all of them reach MIN_MARGIN."""
    chosen = {}
    for kind in KINDS:
        cands, t = [], 0
        while True:
            while t < tries:
                tag = f"dac-eval-{kind}-{t}"
                pcm = clip(kind, tag)
                m = min_margin(model, ref, pcm)
                print(f"   candidate {tag}: min margin {m:.3e}")
                cands.append((m, tag, pcm))
                t += 1
            cands.sort(key=lambda c: -c[0])
            if cands[per_kind - 1][0] >= MIN_MARGIN:
                break
            assert tries < max_tries, f"no {per_kind} {kind} clips with a margin of {MIN_MARGIN} among {tries} candidates"
            tries += 6
        chosen[kind] = cands[:per_kind]
    return [chosen[kind][i] for i in range(per_kind) for kind in KINDS]          # noise, voiced, noise, voiced


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else ref_shims.REFERENCE_ROOT
    torch.manual_seed(0)
    torch.set_num_threads(8)
    metrics = reference_metrics(ref_root)
    mod = gdg.load_reference_dac(ref_root)
    cfg = gdg.CONFIGS[NAME][0]
    model = mod.DAC(**cfg).eval()
    manifest = {k: list(v.shape) for k, v in model.state_dict().items()}
    sd = {k: torch.from_numpy(v) for k, v in gdg.synth.dac_state_dict(manifest).items()}
    model.load_state_dict(sd, strict=True)
    ref = gdg.du.DacRef(cfg, sd)
    clips = pick(model, ref)
    margin = min(c[0] for c in clips)
    assert margin >= MIN_MARGIN, margin
    pcm = np.stack([c[2] for c in clips])
    x = torch.from_numpy(gdg.synth.pcm_to_float(pcm))[:, :-80]       # EvalSet drops the last 80 samples
    batches = [x[:2], x[2:]]
    funcs = {"MelDistance": metrics.MelSpectrogramDistance(), "SISDR": metrics.SISDR()}
    ec = metrics.EntropyCounter(cfg["codebook_size"], num_streams=max(NS), num_groups=1, device="cpu")
    table = {name: [] for name in funcs}
    table["utilization"] = []
    with torch.no_grad():
        codes18 = torch.cat([model(xb[:, None], cfg["sample_rate"], max(NS))["codes"] for xb in batches])
        for n in NS:
            scores = {name: [] for name in funcs}
            ec.reset_stats(num_streams=n)
            for xb in batches:
                out = model(xb[:, None], cfg["sample_rate"], n)
                assert out["audio"].shape[-1] == N_SAMPLES - 80 and out["codes"].shape[1] == n
                for name, fn in funcs.items():
                    scores[name] += fn(xb, out["audio"][:, 0]).tolist()
                ec.update(out["codes"][:, :, None])
            for name, vals in scores.items():
                table[name].append(round(float(np.mean(vals)), 4))
            table["utilization"].append(ec.compute_utilization()[0])
            print(f"   n = {n:2d}: " + " | ".join(f"{k}: {v[-1]}" for k, v in table.items()))
    out = {"config_name": np.array(NAME), "pcm": pcm, "clip_tags": np.array(json.dumps([c[1] for c in clips])), "min_margin": np.float64(margin),
           "n_quantizers": np.array(NS, dtype=np.int64), "codes_n18": codes18.numpy().astype(np.int16), "eval_json": np.array(json.dumps(table))}
    path = os.path.join(gdg.GOLD, "dac_eval.npz")
    np.savez_compressed(path, **out)
    sz = os.path.getsize(path)
    print(f"wrote {path} ({sz / 1e3:.0f} kB), min margin {margin:.3e}")
    assert sz < 1 << 20, "fixture above the 1 MiB limit for a committed file"


if __name__ == "__main__":
    main()
