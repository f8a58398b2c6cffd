"""TEST INFRASTRUCTURE -- the rvq+swinT codec (RVQCodecs): generates tests/golden/rvq_{tiny,base}.npz and their manifests by running the
REAL reference (/root/reference, imported through oracle/ref_shims.py) with name-keyed deterministic weights (esc/synth.py) on int16 PCM inputs
that are stored inside each fixture.  Reuses oracle/gen_golden.py's build_reference(..., name="rvq+swinT") and MarginTap unchanged.  Run in
the build container only:

    python tools/gen_rvq_golden.py

Each fixture holds the inputs, the codes at every S (and asserts the prefix property), the eval-forward cm_loss / cb_loss at every S, the audio
at a few S, the per-(vector, group, stage) argmin margins of the reference's own search, and the projected bottleneck vectors (B, T, G, d) that
the tests continue the restatement from after a near-tie.  Data only; no reference source is stored.
"""
import json
import os
import sys

import numpy as np
import torch
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gen_golden as gg  # noqa: E402  (build_reference, MarginTap, synth, ref_shims)

GOLD = os.path.join(ROOT, "tests", "golden")

RVQ_TINY_CFG = dict(in_dim=2, in_freq=48, h_dims=[8, 12, 16], max_streams=3, win_len=5, hop_len=1.25, sr=16000, patch_size=[3, 2],
                    swin_heads=[2, 4], swin_depth=2, window_size=4, mlp_ratio=4.0, overlap=2, num_rvqs=4, group_size=3, codebook_dim=4,
                    codebook_size=64, l2norm=True, backbone="transformer")


def margins_of(tap, groups, stages):
    """MarginTap rows of one quantizers.encode call arrive group-major, stage-minor (quantization.py:373-376 -> 230-243): (B, S, G, T)."""
    rows, tap.rows = tap.rows, []
    assert len(rows) == groups * stages, (len(rows), groups, stages)
    return torch.stack([torch.stack([rows[m * stages + i] for m in range(groups)], dim=1) for i in range(stages)], dim=1)


def projected(model, x):
    """The bottleneck vectors after each group's proj_down, (B, T, G, d) (quantization.py:367-372)."""
    from esc.modules.vq.quantization import pre_process
    q = model.quantizers
    with torch.no_grad():
        enc_hs, _ = model.encoder(model.spec_transform(x))
        z = pre_process(enc_hs[-1], q.in_freq, q.overlap, q.fix_dim, 3)
        out, s = [], 0
        for m, rvq in enumerate(q.vqs):
            out.append(rvq.proj_down(z[..., s:s + q.vq_dims[m]]))
            s += q.vq_dims[m]
    return torch.stack(out, dim=2)


def pick(model, tap, cfg, n_samples, kinds, tries=6):
    """Per kind, the clip (of `tries` candidates) whose smallest reference margin over every stage is largest."""
    G, S = cfg["group_size"], cfg["num_rvqs"]
    chosen = []
    for kind in kinds:
        best = None
        for t in range(tries):
            tag = f"rvq-{kind}-{t}"
            pcm = (gg.synth.noise_clip_int16 if kind == "noise" else gg.synth.voiced_clip_int16)(tag, n_samples)
            model.encode(torch.from_numpy(gg.synth.pcm_to_float(pcm))[None], num_streams=S)
            m = float(margins_of(tap, G, S).min())
            print(f"   candidate {tag}: min margin {m:.3e}")
            if best is None or m > best[0]:
                best = (m, tag, pcm)
        chosen.append(best)
    return chosen


def fixture(ref_models, tap, cfg, n_samples, kinds, full_audio, dec_audio):
    G, S = cfg["group_size"], cfg["num_rvqs"]
    model, manifest = gg.build_reference(ref_models, cfg, name="rvq+swinT")
    clips = pick(model, tap, cfg, n_samples, kinds)
    pcm = np.stack([c[2] for c in clips])
    x = torch.from_numpy(gg.synth.pcm_to_float(pcm))
    out = {"pcm": pcm, "config_json": np.array(json.dumps(cfg)), "model_name": np.array("rvq+swinT"),
           "clip_tags": np.array(json.dumps([c[1] for c in clips]))}
    with torch.no_grad():
        codes_full, shape = model.encode(x, num_streams=S)
    out["margins"] = margins_of(tap, G, S).numpy().astype(np.float32)
    out["feat_shape"] = np.array(shape, dtype=np.int64)
    out["codes"] = codes_full.numpy().astype(np.int16)
    out["z_proj"] = projected(model, x).numpy().astype(np.float32)
    for s in range(1, S + 1):
        with torch.no_grad():
            codes, shp = model.encode(x, num_streams=s)
            tap.rows = []
            assert tuple(shp) == tuple(shape) and torch.equal(codes, codes_full[:, :s]), "prefix property violated in the reference"
            fw = model(**dict(x=x, x_feat=None, num_streams=s))
            tap.rows = []
            assert torch.equal(fw["codes"], codes)
        out[f"codes_s{s}"] = codes.numpy().astype(np.int16)
        out[f"cm_loss_s{s}"] = fw["cm_loss"].numpy().astype(np.float32)
        out[f"cb_loss_s{s}"] = fw["cb_loss"].numpy().astype(np.float32)
        if s in full_audio or s in dec_audio:
            with torch.no_grad():
                audio = model.decode(codes, shape)
            assert torch.equal(fw["recon_audio"], audio), "forward(eval) != decode(encode()) in the reference"
            a = audio.numpy().astype(np.float32)
            out[f"audio_s{s}"] = a if s in full_audio else a[:, ::8].copy()
            out[f"audio_rms_s{s}"] = np.sqrt((a.astype(np.float64) ** 2).mean(axis=1))
    with torch.no_grad():      # S above num_rvqs: the reference returns num_rvqs streams
        over, _ = model.encode(x, num_streams=S + 2)
        tap.rows = []
    assert torch.equal(over, codes_full)
    return out, manifest, float(model.max_bps)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    ref_models = gg.ref_shims.load_reference()
    tap = gg.MarginTap()
    base_cfg = yaml.safe_load(open(f"{gg.ref_shims.REFERENCE_ROOT}/configs/ablations/9kbps_rvq_swinT.yaml"))["model"]
    summary = {}
    for name, cfg, n, kinds, full, dec in (("rvq_tiny", RVQ_TINY_CFG, 1280, ["noise", "voiced"], (1, 2, 3, 4), ()),
                                           ("rvq_base", base_cfg, 48000, ["noise", "voiced"], (6,), (1, 3))):
        print(f"[{name}]")
        out, manifest, max_bps = fixture(ref_models, tap, cfg, n, kinds, full, dec)
        out["max_bps"] = np.array(max_bps)
        path = os.path.join(GOLD, f"{name}.npz")
        np.savez_compressed(path, **out)
        json.dump(manifest, open(os.path.join(GOLD, f"{name}_manifest.json"), "w"), indent=0)
        summary[name] = dict(keys=len(manifest), max_bps=max_bps, min_margin=float(out["margins"].min()), bytes=os.path.getsize(path))
        print(json.dumps(summary[name]))
    tap.close()


if __name__ == "__main__":
    main()
