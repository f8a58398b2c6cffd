"""TEST INFRASTRUCTURE -- DAC's chunked compress / decompress (esc.baselines.DAC.compress): generates tests/golden/dac_chunk.npz by running the
REAL reference DAC (baselines/descript of the reference repository) on the CPU with `model.padding = False`.  Run in the build container only:

    python tools/gen_dac_chunk_golden.py [REFERENCE_ROOT]

The reference is imported the way tools/gen_dac_golden.py does (a stub `dac` package over the reference's files, stubs of audiotools), with the
same synthetic state (esc.synth.dac_state_dict) and noise clips (esc.synth.noise_clip_int16).  audiotools.AudioSignal is absent, so the loop of
CodecMixin.compress / decompress (base.py:182-233, 259-274) is restated here around the reference model's own get_delay / get_output_length /
preprocess / encode / quantizer.from_codes / decode; resampling, loudness and normalisation are not part of it.  Per case (tests/dac_chunk_util.py
CASES) the fixture holds the int16 PCM, delay / hop / n_samples / chunk_length / chunk count, the concatenated codes, the per-chunk z, the
concatenated reconstruction before trimming and the reference's per-code argmin margins; plus delay and get_output_length of the three
configurations.  Every margin is asserted to be at least 1e-5, so the tests demand strict code equality.  Data only; no reference source is stored.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
from esc import synth  # noqa: E402
import dac_chunk_util as cu  # noqa: E402
import gen_dac_golden as gd  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
MIN_MARGIN = 1e-5


def reference_model(mod, name):
    cfg = gd.CONFIGS[name][0]
    model = mod.DAC(**cfg).eval()
    manifest = {k: list(v.shape) for k, v in model.state_dict().items()}
    sd = {k: torch.from_numpy(synth.dac_state_dict({k: s})[k]) for k, s in manifest.items()}
    model.load_state_dict(sd, strict=True)
    return cfg, model, sd


def case(model, cfg, sd, key, win_duration, nt):
    ref = cu.DacRefNoPad(cfg, sd)
    pcm = np.stack([synth.noise_clip_int16(cu.clip_tag(key), nt)])
    x = torch.from_numpy(synth.pcm_to_float(pcm))[:, None]
    sr, hop_length = cfg["sample_rate"], int(model.hop_length)
    assert nt / sr > win_duration, "the chunked branch is the one under test"
    model.padding = False
    try:
        delay = int(model.delay)
        n_samples = int(math.ceil(int(win_duration * sr) / hop_length) * hop_length)
        hop = int(model.get_output_length(n_samples))
        xp = torch.nn.functional.pad(x, (delay, delay))
        codes, zs, margins, wins = [], [], [], []
        with torch.no_grad():
            for i in range(0, nt, hop):
                w = xp[..., i:i + n_samples]
                w = torch.nn.functional.pad(w, (0, max(0, n_samples - w.shape[-1])))
                w = model.preprocess(w, sr)
                z, c, _, _, _ = model.encode(w, None)
                rz, rc, _, _, _, mg = ref.quantize(ref.encoder(w), None, margins=True)
                assert torch.equal(rc, c), "restatement codes differ from the reference"
                assert cu.rel(rz, z) < 1e-5
                codes.append(c); zs.append(z); margins.append(mg); wins.append(w)
                chunk_length = c.shape[-1]
            assert torch.equal(torch.cat(wins, 0), cu.chunk_batch(x, delay, hop, n_samples)), "the test helper cuts other windows"
            codes_cat = torch.cat(codes, dim=-1)
            recons = []
            for i in range(0, codes_cat.shape[-1], chunk_length):
                zq = model.quantizer.from_codes(codes_cat[..., i:i + chunk_length])[0]
                r = model.decode(zq)
                assert r.shape[-1] == hop, "a chunk decodes to exactly the hop"
                assert cu.rel(ref.decoder(zq), r) < 1e-5
                recons.append(r)
            recon = torch.cat(recons, dim=-1)
            assert recon.shape[-1] >= nt
    finally:
        model.padding = True
    margins = torch.cat(margins, dim=-1).numpy().astype(np.float32)
    assert float(margins.min()) >= MIN_MARGIN, f"{key}: margin {float(margins.min()):.3e} below {MIN_MARGIN}: choose another clip"
    print(f"[{key}] n_samples {n_samples} hop {hop} delay {delay} chunks {len(codes)} chunk_length {chunk_length}  min margin {float(margins.min()):.3e}")
    return {f"{key}_pcm": pcm, f"{key}_geometry": np.array([delay, hop, n_samples, chunk_length, len(codes)], dtype=np.int64),
            f"{key}_codes": codes_cat.numpy().astype(np.int16), f"{key}_z": torch.cat(zs, 0).numpy().astype(np.float32),
            f"{key}_recon": recon.numpy().astype(np.float32), f"{key}_margins": margins}


def main():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_shims
    ref_root = sys.argv[1] if len(sys.argv) > 1 else ref_shims.REFERENCE_ROOT
    torch.manual_seed(0)
    torch.set_num_threads(8)
    mod = gd.load_reference_dac(ref_root)
    out, models = {}, {}
    for name, ns in cu.GEOMETRY_NS.items():
        cfg, model, sd = reference_model(mod, name)
        models[name] = (cfg, model, sd)
        out[f"{name}_delay"] = np.array([int(model.get_delay())], dtype=np.int64)
        out[f"{name}_output_length"] = np.array([[n, int(model.get_output_length(n))] for n in ns], dtype=np.int64)
        print(f"[{name}] delay {int(out[f'{name}_delay'][0])}  get_output_length {out[f'{name}_output_length'].tolist()}")
    for key, name, win, nt in cu.CASES:
        cfg, model, sd = models[name]
        out.update(case(model, cfg, sd, key, win, nt))
    path = os.path.join(GOLD, "dac_chunk.npz")
    np.savez_compressed(path, **out)
    sz = os.path.getsize(path)
    print(f"   wrote {path} ({sz / 1e3:.0f} kB)")
    assert sz < 1 << 20, "fixture above the 1 MiB limit for a committed file"


if __name__ == "__main__":
    main()
