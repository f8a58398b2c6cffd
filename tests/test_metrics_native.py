"""The length-aware evaluation metrics on the GPU (esc.metrics -> escx_mel_distance / escx_sisdr_metric / escx_code_histogram) and the ragged
evaluation harness (scripts/test.py --ragged) against the reference's per-clip semantics: the scripts.metrics classes in float64 on x[b, :L_b] and
y[b, :L_b] alone (tests/metrics_util.py; test_metrics_native_host.py checks the cases' conditioning on the CPU)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
import loss_util as LU  # noqa: E402
import metrics_util as MU  # noqa: E402

pytestmark = pytest.mark.gpu

HARNESS_ATOL = 2e-3             # tests/test_eval_harness.py:116-117
SISDR_TOL = dict(rtol=1e-5, atol=1e-4)          # tests/test_eval_harness.py:20


def _nm():
    from esc import metrics as NM
    return NM


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


# ---- mel distance -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", MU.MEL_UNIFORM)
def test_mel_distance_uniform(B, L):
    x, y = MU.mel_pair(B, L)
    d = _nm().MelSpectrogramDistance().cuda()
    got = d(x.cuda(), y.cuda())
    assert got.shape == (B,) and got.dtype == torch.float32 and got.is_cuda
    f64, _ = MU.mel_reference(B, L)
    err = LU.rel_err(got.cpu().numpy(), f64)
    print(f"B={B} L={L}: relative error to float64 {err:.2e}")
    assert err <= LU.LOSS_RTOL
    same = d(x.cuda(), x.clone().cuda())
    assert (same == 0).all(), "identical inputs give exactly 0"


@pytest.mark.parametrize("lengths", MU.MEL_RAGGED_LENGTHS, ids=lambda v: "-".join(map(str, v)))
def test_mel_distance_ragged(lengths):
    B, N = 3, MU.MEL_N
    x, y = MU.mel_pair(B, N)
    d = _nm().MelSpectrogramDistance().cuda()
    xc, yc = x.cuda(), y.cuda()
    got = d(xc, yc, lengths=lengths)
    f64, _ = MU.mel_reference(B, N, tuple(lengths))
    for b in range(B):
        err = abs(float(got[b]) - f64[b]) / f64[b]
        print(f"lengths={lengths} clip {b}: relative error to float64 on the clip alone {err:.2e}")
        assert err <= LU.LOSS_RTOL, (b, float(got[b]), f64[b])
    assert np.array_equal(_bits(d(xc, yc, lengths=torch.tensor(lengths))), _bits(got)), "two calls are bitwise equal"
    # nothing at or past len[b] is read, whatever it holds
    assert np.array_equal(_bits(d(MU.poison(x, lengths).cuda(), MU.poison(y, lengths).cuda(), lengths=lengths)), _bits(got))
    # clip 0 does not depend on the other clips or their lengths
    x2, y2 = x.clone(), y.clone()
    x2[1:] = torch.flip(x[1:], dims=(1,)) * 0.3; y2[1:] = 0.0
    other = [lengths[0], 1025 if lengths[1] != 1025 else 3000, MU.MEL_N if lengths[2] != MU.MEL_N else 1500]
    assert np.array_equal(_bits(d(x2.cuda(), y2.cuda(), lengths=other))[0], _bits(got)[0])


def test_mel_distance_full_lengths_equal_the_plain_call():
    B, N = 3, MU.MEL_N
    x, y = MU.mel_pair(B, N)
    d = _nm().MelSpectrogramDistance().cuda()
    plain, full = d(x.cuda(), y.cuda()), d(x.cuda(), y.cuda(), lengths=[N] * B)
    assert LU.rel_err(full.cpu().numpy(), plain.cpu().numpy().astype(np.float64)) <= LU.LOSS_RTOL


def test_mel_distance_refuses_bad_arguments_in_the_library():
    """The C entry point checks on its own (the Python class checks first): a length outside (1024, n_samples] is named with its clip."""
    import ctypes
    from esc import _native
    lib = _native.load()
    x = torch.zeros(2, 2048, device="cuda")
    out = torch.empty(2, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    bad = (ctypes.c_int32 * 2)(2048, 1024)
    assert lib.escx_mel_distance(x.data_ptr(), x.data_ptr(), 2, 2048, bad, 16000, out.data_ptr(), st) == _native.ESCX_ERR_INVALID_ARG
    assert b"lengths[1]=1024" in lib.escx_last_error()
    assert lib.escx_mel_distance(x.data_ptr(), x.data_ptr(), 2, 1024, None, 16000, out.data_ptr(), st) == _native.ESCX_ERR_INVALID_ARG
    assert lib.escx_mel_distance(None, x.data_ptr(), 2, 2048, None, 16000, out.data_ptr(), st) == _native.ESCX_ERR_INVALID_ARG
    assert lib.escx_mel_distance(x.data_ptr(), x.data_ptr(), 0, 2048, None, 16000, out.data_ptr(), st) == _native.ESCX_ERR_INVALID_ARG
    assert lib.escx_sisdr_metric(x.data_ptr(), x.data_ptr(), 2, 2048, (ctypes.c_int32 * 2)(0, 5), 1, 1, out.data_ptr(), st) == _native.ESCX_ERR_INVALID_ARG
    assert b"lengths[0]=0" in lib.escx_last_error()
    assert lib.escx_code_histogram(None, 1, 1, 1, 1, 4, out.data_ptr(), out.data_ptr(), st) == _native.ESCX_ERR_INVALID_ARG


# ---- SI-SDR -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaling,zero_mean", MU.SISDR_MODES)
def test_sisdr_ragged(scaling, zero_mean):
    x, y = MU.sisdr_pair()
    lengths = MU.SISDR_LENGTHS
    f = _nm().SISDR(scaling=scaling, zero_mean=zero_mean).cuda()
    got = f(x.cuda(), y.cuda(), lengths=lengths)
    assert got.shape == (len(lengths),) and got.dtype == torch.float32
    ref = MU.sisdr_reference(scaling, zero_mean)
    print(f"scaling={scaling} zero_mean={zero_mean}: got {got.cpu().numpy()} float64 {ref}")
    np.testing.assert_allclose(got.cpu().numpy(), ref, **SISDR_TOL)
    assert np.array_equal(_bits(f(MU.poison(x, lengths).cuda(), MU.poison(y, lengths).cuda(), lengths=lengths)), _bits(got))
    assert np.array_equal(_bits(f(x.cuda(), y.cuda(), lengths=lengths)), _bits(got))
    # lengths=None is the reference's class on the whole rows
    from scripts import metrics as M
    whole = M.SISDR(scaling=scaling, zero_mean=zero_mean)(x.double(), y.double()).numpy()
    np.testing.assert_allclose(f(x.cuda(), y.cuda()).cpu().numpy(), whole, **SISDR_TOL)


def test_sisdr_identical_inputs_give_the_reference_inf():
    from scripts import metrics as M
    x, _ = MU.sisdr_pair()
    assert torch.isposinf(M.SISDR()(x.double(), x.double())).all()
    got = _nm().SISDR().cuda()(x.cuda(), x.clone().cuda(), lengths=[n for n in MU.SISDR_LENGTHS])
    assert torch.isposinf(got).all(), got


# ---- histogram ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", MU.HIST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_code_histogram(shape):
    B, S, G, T, K = shape
    codes, live = MU.hist_codes(shape)
    ec = _nm().EntropyCounter(K, num_streams=S, num_groups=G, device="cuda")
    ec.update(codes.cuda())
    counts, (rate, util) = MU.hist_reference(shape)
    assert torch.equal(ec.counts.cpu(), counts) and ec.total_counts == sum(live)
    assert ec.compute_utilization() == (rate, util)
    ec.update(codes.cuda())                                            # accumulation over two calls
    counts2, ref2 = MU.hist_reference(shape, repeats=2)
    assert torch.equal(ec.counts.cpu(), counts2) and ec.total_counts == 2 * sum(live) and ec.compute_utilization() == ref2
    planted = codes.clone()
    planted[0, S - 1, G - 1, 0] = K
    ec.reset_stats(S)
    with pytest.raises(ValueError, match="at or above codebook_size"):
        ec.update(planted.cuda())
    assert ec.total_counts == 0


# ---- the harness ----------------------------------------------------------------------------------------------------------------------------------------
def _run_cli(monkeypatch, folder, out, extra):
    from scripts import test as T
    monkeypatch.setattr(sys, "argv", ["scripts.test", "--eval_folder_path", str(folder), "--save_path", str(out), "--device", "cuda"] + extra)
    table = T.run(T.parse_args())
    assert json.load(open(os.path.join(out, "perf_stats.json"))) == table
    return table


def _per_file_loop(model, folder, slots_of):
    """The reference's way: every snapped file alone through the plain call and the scripts.metrics classes.  Returns the table and, per bitrate, the codes per file."""
    from scripts import metrics as M
    from scripts import utils as U
    mel, sdr = M.MelSpectrogramDistance().cuda(), M.SISDR().cuda()
    files = sorted(os.listdir(folder))
    table, all_codes = {"MelDistance": [], "SISDR": [], "utilization": []}, []
    for s in range(1, model.max_streams + 1):
        ec = M.EntropyCounter(slots_of["K"], num_streams=slots_of["slots"](s), num_groups=slots_of["G"], device="cuda")
        vals, codes = {"MelDistance": [], "SISDR": []}, []
        for f in files:
            w = U.load_wav(os.path.join(folder, f))[0][0]
            x = w[None, :U.snap_length(model, w.shape[0])].cuda()
            with torch.no_grad():
                out = model(x=x, x_feat=None, num_streams=s)
            vals["MelDistance"] += mel(x, out["recon_audio"]).tolist(); vals["SISDR"] += sdr(x, out["recon_audio"]).tolist()
            ec.update(out["codes"]); codes.append(out["codes"].cpu())
        for k, v in vals.items():
            table[k].append(round(float(np.mean(v)), 4))
        table["utilization"].append(ec.compute_utilization()[0])
        all_codes.append(codes)
    return table, all_codes


def _assert_batch_codes_equal(model, folder, all_codes):
    """The ragged batch's codes, clip by clip, are the codes of the file alone (asserted first: utilisation and metrics follow from it)."""
    from scripts import utils as U
    x, lengths, indices = U.ragged_collate([U.RaggedEvalSet(str(folder), model)[i] for i in range(len(all_codes[0]))])
    files = sorted(os.listdir(folder))
    for s in range(1, model.max_streams + 1):
        with torch.no_grad():
            out = model(x=x.cuda(), x_feat=None, num_streams=s, lengths=lengths)
        assert out["recon_audio"].shape == x.shape
        for b, k in enumerate(indices):
            alone = all_codes[s - 1][k]
            got = out["codes"][b:b + 1, :, :, :alone.shape[-1]].cpu()
            assert torch.equal(got, alone), f"{files[k]} (bitrate {s}): {int((got != alone).sum())} of {alone.numel()} codes differ from the file's own call"
            assert (out["codes"][b, :, :, alone.shape[-1]:] == -1).all()


def _check_tables(got, ref, n_rates):
    assert set(got) == {"MelDistance", "SISDR", "utilization"} and all(len(v) == n_rates for v in got.values())       # the layout of scripts/test.py:81
    assert got["utilization"] == ref["utilization"]
    np.testing.assert_allclose(got["SISDR"], ref["SISDR"], atol=HARNESS_ATOL)
    np.testing.assert_allclose(got["MelDistance"], ref["MelDistance"], atol=HARNESS_ATOL)


def test_ragged_harness_dac(tmp_path, monkeypatch):
    """--ragged --synthetic dac_tiny on four files of 0.3 to 1.0 s against the per-file loop: DAC's lengths contract is bitwise, so the codes are equal."""
    import argparse
    from scripts import test as T
    folder = MU.write_wavs(str(tmp_path / "wavs"), MU.DAC_CLIPS)
    model = T.load_dac(argparse.Namespace(dac_path=None, synthetic="dac_tiny", n_quantizers=None)).cuda()
    ref, codes = _per_file_loop(model, folder, {"K": model.dac.codebook_size, "G": 1, "slots": model.code_slots})
    _assert_batch_codes_equal(model, folder, codes)
    got = _run_cli(monkeypatch, folder, tmp_path / "out", ["--ragged", "--batch_size", "4", "--synthetic", "dac_tiny"])
    print("ragged:", got, "\nper file:", ref)
    _check_tables(got, ref, model.max_streams)


def test_ragged_harness_esc(tmp_path, monkeypatch):
    """--ragged --synthetic tiny (fp32) on four files against the per-file loop.  The clips (metrics_util.ESC_CLIPS: voiced "ragged-eval-voiced-1" 4800
    samples, noise "ragged-eval-noise-3" 7013, voiced "ragged-eval-voiced-0" 11111, noise "ragged-eval-noise-3" 16000; snapped 4780 / 6940 / 11100 /
    15980) have smallest CPU-oracle argmin margins over all streams of 4.04e-4, 1.53e-4, 9.06e-5 and 7.22e-5, all above 1e-5 = 5 x NEAR_TIE, so no
    code may differ between the batch and the file alone; batch_size 3 makes two batches, the second a single clip."""
    import argparse
    from scripts import test as T
    monkeypatch.setenv("ESCX_PRECISION", "fp32")
    folder = MU.write_wavs(str(tmp_path / "wavs"), MU.ESC_CLIPS)
    model, cfg = T.load_model(argparse.Namespace(model_path=None, synthetic="tiny"))
    model = model.cuda().eval()
    assert model.precision == "fp32"
    ref, codes = _per_file_loop(model, folder, {"K": cfg["codebook_size"], "G": cfg["group_size"], "slots": lambda s: s})
    _assert_batch_codes_equal(model, folder, codes)
    got = _run_cli(monkeypatch, folder, tmp_path / "out", ["--ragged", "--batch_size", "3", "--synthetic", "tiny"])
    print("ragged:", got, "\nper file:", ref)
    _check_tables(got, ref, cfg["max_streams"])


def test_native_metrics_on_a_uniform_folder(tmp_path, monkeypatch):
    """--native_metrics alone swaps the metric classes on the uniform path: the table of the plain run within the harness tolerance."""
    from scipy.io import wavfile
    from esc import synth
    d = tmp_path / "wavs"; d.mkdir()
    for i in range(3):
        wavfile.write(d / f"clip{i}.wav", 16000, synth.voiced_clip_int16(f"eval-{i}", 48000))
    common = ["--batch_size", "3", "--synthetic", "base"]
    plain = _run_cli(monkeypatch, d, tmp_path / "plain", common)
    native = _run_cli(monkeypatch, d, tmp_path / "native", common + ["--native_metrics"])
    print("native:", native, "\nplain:", plain)
    _check_tables(native, plain, 6)
