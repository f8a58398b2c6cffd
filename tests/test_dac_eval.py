"""The evaluation harness's DAC arm and its one-pass sweep on the MI355X (efficient-speech-codec_amd/scripts/test.py): eval_epoch through
DacEvalModel against the table the real reference DAC and the reference's metric classes give on the same clips
(tools/gen_dac_eval_golden.py), eval_epoch_one_pass against eval_epoch for DAC, ESC and RVQCodecs (identical tables), ESC-Base one-pass
against the reference's own eval_epoch, and the command-line entry with --synthetic dac_syn --one_pass."""
import json
import os
import sys
import types

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, load_golden, load_manifest, synth_state

sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
from esc import synth  # noqa: E402
from scripts import metrics as M  # noqa: E402

pytestmark = pytest.mark.gpu


def _funcs():
    return {"MelDistance": M.MelSpectrogramDistance().cuda(), "SISDR": M.SISDR().cuda()}


@pytest.fixture(scope="module")
def dac_arm():
    """(adapter around dac_tiny with synthetic weights, the fixture, its four clips as EvalSet serves them, in two batches of two)."""
    from esc.baselines import DAC
    from scripts.test import DacEvalModel
    g = np.load(os.path.join(GOLDEN, "dac_eval.npz"))
    name = str(g["config_name"])
    dac = DAC(**json.loads(str(load_golden(name)["config_json"])))
    dac.load_state_dict({k: torch.from_numpy(v) for k, v in synth.dac_state_dict(load_manifest(name)).items()}, strict=True)
    x = torch.from_numpy(synth.pcm_to_float(g["pcm"]))[:, :-80]
    return DacEvalModel(dac.cuda().eval(), [int(n) for n in g["n_quantizers"]]), g, [x[:2], x[2:]]


def _dac_counter(model):
    return M.EntropyCounter(model.dac.codebook_size, num_streams=model.code_slots(model.max_streams), num_groups=1, device="cuda")


def test_dac_arm_against_the_reference_table(dac_arm):
    from scripts.test import eval_epoch
    model, g, batches = dac_arm
    ref = json.loads(str(g["eval_json"]))
    out = eval_epoch(model, batches, _funcs(), _dac_counter(model), "cuda", model.bps_per_stream, verbose=False)
    codes = torch.cat([model(x=x.cuda(), x_feat=None, num_streams=model.max_streams)["codes"] for x in batches])
    print("device   ", out)
    print("reference", ref)
    print("codes equal to the reference's at 18 codebooks:", np.array_equal(codes[:, :, 0].cpu().numpy(), g["codes_n18"].astype(np.int64)))
    assert model.bps_per_stream == pytest.approx(1.5) and list(out) == ["MelDistance", "SISDR", "utilization"]
    assert codes.shape == (4, 18, 1, 50)
    assert out["utilization"] == ref["utilization"]
    np.testing.assert_allclose(out["SISDR"], ref["SISDR"], atol=2e-3)
    np.testing.assert_allclose(out["MelDistance"], ref["MelDistance"], atol=2e-3)


def test_one_pass_equals_sequential_dac(dac_arm):
    from scripts.test import eval_epoch, eval_epoch_one_pass
    model, g, batches = dac_arm
    seq = eval_epoch(model, batches, _funcs(), _dac_counter(model), "cuda", 1.5, verbose=False)
    one = eval_epoch_one_pass(model, batches, _funcs(), _dac_counter(model), "cuda", 1.5, verbose=False)
    assert one == seq and len(one["SISDR"]) == 6
    assert eval_epoch_one_pass(model, batches, _funcs(), _dac_counter(model), "cuda", 1.5, num_streams=4, verbose=False) == \
        eval_epoch(model, batches, _funcs(), _dac_counter(model), "cuda", 1.5, num_streams=4, verbose=False)


@pytest.mark.parametrize("name", ["tiny", "rvq_tiny"])
def test_one_pass_equals_sequential_esc_and_rvq(name):
    """ESC `tiny` and RVQCodecs `rvq_tiny` on four 1260-sample clips (64 frames: the reconstruction has the input's length)."""
    from esc.models import make_model
    from scripts.test import eval_epoch, eval_epoch_one_pass
    g = load_golden(name)
    cfg = json.loads(str(g["config_json"]))
    model = make_model(cfg, str(g["model_name"]) if "model_name" in g else "csvq+swinT")
    model.load_state_dict(synth_state(name), strict=True)
    model = model.cuda().eval()
    pcm = np.stack([(synth.voiced_clip_int16 if i % 2 else synth.noise_clip_int16)(f"one-pass-{name}-{i}", 1260) for i in range(4)])
    x = torch.from_numpy(synth.pcm_to_float(pcm))
    batches = [x[:2], x[2:]]
    ec = M.EntropyCounter(cfg["codebook_size"], num_streams=cfg["max_streams"], num_groups=cfg["group_size"], device="cuda")
    seq = eval_epoch(model, batches, _funcs(), ec, "cuda", 1.5, verbose=False)
    one = eval_epoch_one_pass(model, batches, _funcs(), ec, "cuda", 1.5, verbose=False)
    print(seq)
    assert one == seq and len(one["SISDR"]) == model.max_streams and len(set(one["SISDR"])) > 1


def test_esc_base_one_pass_against_the_reference_eval_epoch():
    """tests/test_eval_harness.py::test_eval_loop_on_gpu_matches_reference_eval_epoch with the one-pass sweep: the same clips, the same bounds."""
    from gpu_util import build_models
    from scripts.test import eval_epoch_one_pass
    g = np.load(os.path.join(GOLDEN, "metrics.npz"))
    ref = json.loads(str(g["eval_json"]))
    tags = json.loads(str(g["eval_tags"]))
    model, orc, gb, cfg = build_models("base")
    pcm = np.concatenate([gb["pcm"], np.stack([(synth.noise_clip_int16 if k == "noise" else synth.voiced_clip_int16)(t, 48000) for k, t in tags])])
    x = torch.from_numpy(synth.pcm_to_float(pcm))[:, :-80]
    ec = M.EntropyCounter(cfg["codebook_size"], num_streams=cfg["max_streams"], num_groups=cfg["group_size"], device="cuda")
    out = eval_epoch_one_pass(model, [x[:2], x[2:]], _funcs(), ec, "cuda", 1.5, verbose=False)
    assert not model.training
    assert out["utilization"] == ref["utilization"]
    np.testing.assert_allclose(out["SISDR"], ref["SISDR"], atol=2e-3)
    np.testing.assert_allclose(out["MelDistance"], ref["MelDistance"], atol=2e-3)


def test_cli_dac_arm_one_pass(tmp_path):
    """scripts.test.run with --synthetic dac_syn --one_pass on a folder of wavs: perf_stats.json with one entry per bitrate (4 codebooks: every
    count is a bitrate)."""
    from scipy.io import wavfile
    from scripts.test import run
    d = tmp_path / "wavs"; d.mkdir()
    for i in range(3):
        wavfile.write(d / f"clip{i}.wav", 16000, synth.voiced_clip_int16(f"eval-dac-{i}", 16000))
    args = types.SimpleNamespace(eval_folder_path=str(d), batch_size=2, model_path=None, synthetic="dac_syn", save_path=str(tmp_path / "out"),
                                 device="cuda", one_pass=True)
    table = run(args)
    stats = json.load(open(tmp_path / "out" / "perf_stats.json"))
    assert stats == table and set(stats) >= {"MelDistance", "SISDR", "utilization"}
    assert all(len(v) == 4 for v in stats.values())
    assert all(0.0 <= u <= 1.0 for u in stats["utilization"])
    args.one_pass = False
    assert run(args) == table
