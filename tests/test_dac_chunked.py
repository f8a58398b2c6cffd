"""DAC's chunked compress / decompress on the MI355X (esc.baselines.DAC.padding / compress / decompress, include/escx.h escx_dac_set_padding,
escx_dac_encode_chunks) against the real reference run with `padding = False` (tests/golden/dac_chunk.npz, tools/gen_dac_chunk_golden.py) and the
unpadded torch restatement of tests/dac_chunk_util.py.  Every reference margin of the fixture is at least 1e-5 (asserted by the generator), so
codes are compared for equality with nothing left out."""
import ctypes
import hashlib

import numpy as np
import pytest
import torch

import dac_chunk_util as cu
from conftest import load_golden, load_manifest
from esc import synth

pytestmark = pytest.mark.gpu
IDS = [c[0] for c in cu.CASES]
_MODELS, _REFS = {}, {}


def _sd(name):
    return {k: torch.from_numpy(v) for k, v in synth.dac_state_dict(load_manifest(name)).items()}


def _model(name):
    from esc.baselines import DAC
    if name not in _MODELS:
        m = DAC(**cu.config_of(load_golden, name))
        m.load_state_dict(_sd(name), strict=True)
        _MODELS[name] = m.cuda().eval()
    m = _MODELS[name]
    assert m.padding is True and m.precision == "fp32"          # every test leaves the shared model as it found it
    return m


def _case(case):
    """model, signal (1, 1, nt) on the device, and the fixture's values of one case; the reference results are computed once (the fixture)."""
    key, name, win, nt = case
    g = load_golden("dac_chunk")
    delay, hop, n_samples, chunk_length, n_chunks = (int(v) for v in g[f"{key}_geometry"])
    x = torch.from_numpy(synth.pcm_to_float(g[f"{key}_pcm"]))[:, None]
    assert x.shape == (1, 1, nt)
    ref = dict(delay=delay, hop=hop, n_samples=n_samples, chunk_length=chunk_length, n_chunks=n_chunks, codes=g[f"{key}_codes"].astype(np.int64),
               z=g[f"{key}_z"], recon=g[f"{key}_recon"], win=win, nt=nt, name=name, key=key)
    return _model(name), x.cuda(), ref


def _restated(case):
    """codes, z and audio of the unpadded torch restatement on the window batch of one case (CPU, once per case)."""
    key, name, win, nt = case
    if key not in _REFS:
        _, x, r = _case(case)
        ref = cu.DacRefNoPad(cu.config_of(load_golden, name), _sd(name))
        with torch.no_grad():
            w = cu.chunk_batch(x.cpu(), r["delay"], r["hop"], r["n_samples"])
            z, codes, *_ = ref.encode(w)
            _REFS[key] = (codes.numpy(), z.numpy(), ref.decoder(z).numpy())
    return _REFS[key]


@pytest.mark.parametrize("precision", ("fp32", "bf16x3"))
@pytest.mark.parametrize("case", cu.CASES, ids=IDS)
def test_unpadded_encode_decode_on_the_chunk_batch(case, precision):
    m, x, r = _case(case)
    w = cu.chunk_batch(x, r["delay"], r["hop"], r["n_samples"])
    assert w.shape == (r["n_chunks"], 1, r["n_samples"])
    try:
        m.set_precision(precision)
        m.padding = False
        z, codes, lat, cm, cb = m.encode(w)
        audio = m.decode(z)
        torch.cuda.synchronize()
    finally:
        m.padding = True
        m.set_precision("fp32")
    assert codes.shape == (r["n_chunks"], m.n_codebooks, r["chunk_length"]) and audio.shape == (r["n_chunks"], 1, r["hop"])
    np.testing.assert_array_equal(cu.unchunk_codes(codes, 1).cpu().numpy(), r["codes"])
    ez, ea = cu.rel(z.cpu(), r["z"]), cu.rel_rms(audio.cpu().reshape(1, 1, -1), r["recon"])
    print(f"{r['key']} {precision}: z rel {ez:.2e}, audio rel rms {ea:.2e} against the reference")
    assert ez < 1e-5 and ea < 1e-4
    if precision == "fp32":
        tc, tz, ta = _restated(case)
        np.testing.assert_array_equal(codes.cpu().numpy(), tc)
        ez2, ea2 = cu.rel(z.cpu(), tz), cu.rel_rms(audio.cpu(), ta)
        print(f"{r['key']} fp32: z rel {ez2:.2e}, audio rel rms {ea2:.2e} against the unpadded restatement")
        assert ez2 < 1e-5 and ea2 < 1e-4


@pytest.mark.parametrize("case", cu.CASES, ids=IDS)
def test_compress_reproduces_the_reference_schedule_and_codes(case):
    m, x, r = _case(case)
    f = m.compress(x, win_duration=r["win"])
    assert m.padding is True
    assert (f.chunk_length, f.padding, f.original_length, f.channels, f.sample_rate, f.dac_version) == (r["chunk_length"], False, r["nt"], 1, 16000, "1.0.0")
    assert f.codes.dtype == torch.int64 and f.input_db is None
    np.testing.assert_array_equal(f.codes.cpu().numpy(), r["codes"])
    # the staging kernel against windows cut on the host: the zero fill before the signal, behind it, and in the short last window
    try:
        m.padding = False
        host = cu.unchunk_codes(m.encode(cu.chunk_batch(x, r["delay"], r["hop"], r["n_samples"]))[1], 1)
    finally:
        m.padding = True
    assert torch.equal(f.codes, host)
    for per in (1, 2):
        assert torch.equal(m.compress(x, win_duration=r["win"], chunks_per_pass=per).codes, f.codes), per
    assert torch.equal(m.compress(x[0, 0], win_duration=r["win"]).codes, f.codes)            # (nt,) and (channels, nt) inputs
    assert torch.equal(m.compress(x[0], sample_rate=16000, win_duration=r["win"], n_quantizers=2, input_db=-20.0).codes, f.codes[:, :2])


@pytest.mark.parametrize("case", cu.CASES, ids=IDS)
def test_decompress_of_compress(case, tmp_path):
    from esc.baselines import DACFile
    m, x, r = _case(case)
    f = m.compress(x, win_duration=r["win"], input_db=-20.0)
    y = m.decompress(f)
    assert m.padding is True and y.shape == (1, 1, r["nt"])
    e = cu.rel_rms(y.cpu(), r["recon"][..., :r["nt"]])
    print(f"{r['key']}: reconstruction rel rms {e:.2e} against the reference")
    assert e < 1e-4
    path = f.save(tmp_path / r["key"])
    back = DACFile.load(path)
    assert torch.equal(back.codes, f.codes.cpu()) and back.padding is False and float(back.input_db) == -20.0
    assert torch.equal(m.decompress(path), y) and torch.equal(m.decompress(back, chunks_per_pass=1), y) and torch.equal(m.decompress(f, chunks_per_pass=2), y)


@pytest.mark.parametrize("name,nt,win", (("dac_syn", 768, 0.048), ("dac_syn", 765, 0.048), ("dac_tiny", 16000, 1.0)))
def test_short_signals_take_one_padded_pass(name, nt, win):
    m = _model(name)
    x = torch.from_numpy(synth.pcm_to_float(synth.noise_clip_int16(f"dac-chunk-short-{name}", nt)))[None, None].cuda()
    f = m.compress(x, win_duration=win)
    assert f.padding is True and f.original_length == nt and f.codes.shape[-1] == f.chunk_length == m.num_frames(-(-nt // m.hop_length) * m.hop_length)
    codes = m.encode(m.preprocess(x, None))[1]
    if nt % m.hop_length == 0:
        assert torch.equal(codes, m.encode(x)[1])
    assert torch.equal(f.codes, codes)
    y = m.decompress(f)
    a = m.decode(m.quantizer.from_codes(codes)[0])      # decompress decodes from the codes, as the reference does (base.py:270-271)
    assert y.shape == (1, 1, nt) and m.padding is True
    k = min(nt, a.shape[-1])                            # the padded decoder gives 320 T - 8 (4 T for dac_syn): the rest of original_length is zero
    assert torch.equal(y[..., :k], a[..., :k]) and not bool(y[..., k:].any())
    if name == "dac_tiny":
        assert a.shape[-1] == nt - 8 and k == nt - 8


@pytest.mark.parametrize("precision", ("fp32", "bf16x3"))
def test_channels_and_batch_rows_are_independent(precision):
    """(batch 2, channels 2) through dac_tiny: 12 windows of 16000 samples take the 128-row tiles, a row alone the 64-row ones."""
    case = cu.CASES[3]
    m, x, r = _case(case)
    nt = r["nt"]
    extra = [torch.from_numpy(synth.pcm_to_float(synth.noise_clip_int16(f"dac-chunk-row-{i}", nt))) for i in range(3)]
    sig = torch.stack([x[0, 0].cpu()] + extra).reshape(2, 2, nt).cuda()
    try:
        m.set_precision(precision)
        f = m.compress(sig, win_duration=r["win"])
        y = m.decompress(f)
        assert f.channels == 2 and f.codes.shape == (4, m.n_codebooks, r["n_chunks"] * r["chunk_length"]) and y.shape == (2, 2, nt)
        for i in (0, 3):
            f1 = m.compress(sig.reshape(4, nt)[i], win_duration=r["win"])
            assert torch.equal(f1.codes[0], f.codes[i]), i
            assert torch.equal(m.decompress(f1)[0, 0], y.reshape(4, nt)[i]), i
    finally:
        m.set_precision("fp32")
    if precision == "fp32":
        np.testing.assert_array_equal(f.codes[:1].cpu().numpy(), r["codes"])


def test_padding_is_restored_and_short_inputs_are_refused():
    from esc import _native
    lib = _native.load()
    case = cu.CASES[0]
    m, x, r = _case(case)
    _, hd = m._handle(torch.device("cuda:0"))
    assert lib.escx_dac_get_padding(hd) == 1
    assert lib.escx_dac_delay(hd) == m.delay == r["delay"] and lib.escx_dac_output_length(hd, r["n_samples"]) == r["hop"]
    assert lib.escx_dac_output_length(hd, 0) == m.get_output_length(0) < 0
    assert lib.escx_dac_set_padding(hd, 2) == _native.ESCX_ERR_INVALID_ARG and lib.escx_dac_get_padding(hd) == 1
    try:
        m.padding = False
        assert lib.escx_dac_get_padding(hd) == 0
        m.compress(x, win_duration=r["win"])
        assert m.padding is False and lib.escx_dac_get_padding(hd) == 0          # the previous value, not the default
        with pytest.raises(ValueError):
            m.compress(x, win_duration=0.02)                                       # 320-sample windows: no frame without padding
        assert m.padding is False
        for L in range(1, 400, 7):
            assert lib.escx_dac_num_frames(hd, L) == m.num_frames(L), L
        for T in range(1, 60):
            assert lib.escx_dac_output_samples(hd, T) == m.output_samples(T), T
        short = next(L for L in range(1, 2000) if m.num_frames(L) == 1) - 1
        assert short > m.hop_length and lib.escx_dac_num_frames(hd, short) == 0
        with pytest.raises(ValueError):
            m.encode(torch.zeros(1, 1, short, device="cuda"))
        tmin = next(T for T in range(1, 500) if m.output_samples(T) >= 1)
        with pytest.raises(ValueError):
            m.decode(torch.zeros(1, m.latent_dim, tmin - 1, device="cuda"))
        # the C entry points refuse the same lengths themselves, before the first launch
        flat = m._ensure_flat(torch.device("cuda:0"), lib, hd)
        buf = torch.zeros(1 << 16, device="cuda")
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        p = ctypes.c_void_p(buf.data_ptr())
        assert lib.escx_dac_encode(hd, ctypes.c_void_p(flat.data_ptr()), m._version(), p, 1, short, 4, p, p, p, p, st) == _native.ESCX_ERR_INVALID_ARG
        assert lib.escx_dac_encode_chunks(hd, ctypes.c_void_p(flat.data_ptr()), m._version(), p, 1, 1000, 3, short, 10, 0, 4, p, p, p, p, st) == _native.ESCX_ERR_INVALID_ARG
        assert lib.escx_dac_decode(hd, ctypes.c_void_p(flat.data_ptr()), m._version(), p, 1, tmin - 1, p, st) == _native.ESCX_ERR_INVALID_ARG
        assert m.encode(torch.zeros(1, 1, short + 1, device="cuda"))[1].shape[-1] == 1
        assert m.decode(torch.zeros(1, m.latent_dim, tmin, device="cuda")).shape[-1] == m.output_samples(tmin)
    finally:
        m.padding = True
    assert lib.escx_dac_get_padding(hd) == 1
    with pytest.raises(ValueError):
        m.compress(x, win_duration=0.02)
    assert m.padding is True
    assert m.num_frames(short) >= 1 and lib.escx_dac_num_frames(hd, short) == m.num_frames(short)


def test_snake_placement_is_neutral_without_padding():
    """The cropped residual reads its skip from x while the Snaked copies go through the fourth map: both Snake placements give the same bits."""
    m, x, r = _case(cu.CASES[2])
    from esc import _native
    default = _native.load().escx_dac_get_snake_maps(m._handle(torch.device("cuda:0"))[1])
    w = cu.chunk_batch(x, r["delay"], r["hop"], r["n_samples"])
    try:
        m.padding = False
        z0, c0, *_ = m.encode(w)
        a0 = m.decode(z0)
        for mask in (0, 3, 28):
            m.set_snake_maps(mask)
            z, c, *_ = m.encode(w)
            assert torch.equal(z, z0) and torch.equal(c, c0) and torch.equal(m.decode(z0), a0), mask
    finally:
        m.set_snake_maps(default)
        m.padding = True


# sha256 over codes, z and audio of the calls below, recorded from the parent commit's build (ab73bfd) on an MI355X
PARENT_DAC_TINY_SHA256 = "ac4b8583f2929ec4615b3d2c0be1e0ca38aa875d20e0bf87d720b0fe834a960f"


def default_path_digest(m):
    g = load_golden("dac_tiny")
    x = torch.from_numpy(synth.pcm_to_float(g["pcm"]))[:, None].cuda()
    z, codes, lat, cm, cb = m.encode(x)
    audio = m.decode(z)
    fw = m(torch.from_numpy(synth.pcm_to_float(g["fwd_pcm"]))[:, None].cuda(), n_quantizers=6)
    h = hashlib.sha256()
    for t in (codes, z, lat, audio, fw["codes"], fw["audio"]):
        h.update(np.ascontiguousarray(t.cpu().numpy()).tobytes())
    return h.hexdigest()


def test_default_padding_path_is_bitwise_the_parent_build():
    m = _model("dac_tiny")
    assert default_path_digest(m) == PARENT_DAC_TINY_SHA256
    f = m.compress(torch.zeros(1, 1, 16001, device="cuda"), win_duration=1.0)      # a switch to the unpadded operands and back re-packs both ways
    assert f.padding is False and m.padding is True
    assert default_path_digest(m) == PARENT_DAC_TINY_SHA256


def test_compress_script_writes_the_dac_file_and_the_reconstruction(tmp_path):
    """scripts/compress.py --synthetic dac_tiny: a two-channel 1.5 s wav in 1 s windows; the .dac file decodes to what the script wrote."""
    import os
    import subprocess
    import sys
    from scipy.io import wavfile
    from conftest import ROOT
    from esc.baselines import DACFile
    wav = tmp_path / "in.wav"
    pcm = np.stack([synth.noise_clip_int16("dac-chunk-cli-0", 24000), synth.voiced_clip_int16("dac-chunk-cli-1", 24000)], 1)
    wavfile.write(wav, 16000, pcm)
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "efficient-speech-codec_amd"))
    out = subprocess.run([sys.executable, "-m", "scripts.compress", "--input", str(wav), "--save_path", str(tmp_path / "out"), "--synthetic", "dac_tiny",
                          "--win_duration", "1.0", "--device", "cuda"], capture_output=True, text=True, env=env,
                         cwd=os.path.join(ROOT, "efficient-speech-codec_amd"), timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    f = DACFile.load(tmp_path / "out" / "encoded_in.dac")
    assert (f.channels, f.original_length, f.padding, f.chunk_length, f.sample_rate) == (2, 24000, False, 34, 16000) and f.codes.shape == (2, 18, 5 * 34)
    m = _model("dac_tiny")
    x = torch.from_numpy(synth.pcm_to_float(pcm.T.copy())).cuda()
    assert torch.equal(m.compress(x, win_duration=1.0).codes.cpu(), f.codes)
    sr, rec = wavfile.read(tmp_path / "out" / "decoded_dac_in.wav")
    assert sr == 16000 and rec.shape == (24000, 2)
    np.testing.assert_array_equal(rec, np.clip(m.decompress(f)[0].T.cpu().numpy(), -1, 1))
