"""The DAC baseline codec (esc.baselines.DAC) on the MI355X against the real reference's fixtures (tools/gen_dac_golden.py) and the torch
restatement of tests/dac_util.py: codes under the near-tie rule, z / latents / losses / audio, from_codes, eval forward trimming, the prefix
property, batch independence, in-place parameter changes, the device Snake and tanh, the C-ABI parameter order and uncovered geometries."""
import ctypes
import json

import numpy as np
import pytest
import torch

import dac_util as du
from conftest import load_golden, load_manifest
from esc import synth

pytestmark = pytest.mark.gpu
NAMES = ("dac_syn", "dac_tiny", "dac_base")
_MODELS = {}


def _cfg(name):
    return json.loads(str(load_golden(name)["config_json"]))


def _sd(name):
    return {k: torch.from_numpy(v) for k, v in synth.dac_state_dict(load_manifest(name)).items()}


def _model(name):
    from esc.baselines import DAC
    if name not in _MODELS:
        m = DAC(**_cfg(name))
        m.load_state_dict(_sd(name), strict=True)
        _MODELS[name] = m.cuda().eval()
    return _MODELS[name]


def _x(pcm):
    return torch.from_numpy(synth.pcm_to_float(pcm))[:, None].cuda()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean()) / max(np.sqrt((b ** 2).mean()), 1e-30))


def _check_codes(ref, z_enc, n, got, want, margins):
    got, want = np.asarray(got), np.asarray(want)
    if np.array_equal(got, want):
        return 0
    rows, bad = du.attribute_codes(ref, z_enc, n, got, want, margins[:, :want.shape[1]])
    assert not bad, f"codes differ beyond the near-tie rule: {bad[:5]}"
    return rows


@pytest.mark.parametrize("name", NAMES)
def test_encode_against_the_reference(name):
    g = load_golden(name)
    m = _model(name)
    ref = du.DacRef(_cfg(name), _sd(name))
    x = _x(g["pcm"])
    with torch.no_grad():
        z_enc = ref.encoder(x.cpu())
    for n in du.GOLDEN_NS:
        k = du.nkey(n)
        z, codes, lat, cm, cb = m.encode(x, n)
        torch.cuda.synchronize()
        assert codes.dtype == torch.int64 and cm.dim() == 0 and cb.dim() == 0
        assert codes.shape == g[f"codes_{k}"].shape and lat.shape[1] == codes.shape[1] * m.codebook_dim
        flips = _check_codes(ref, z_enc, n, codes.cpu().numpy(), g[f"codes_{k}"], g["margins"])
        if flips:
            continue                                   # a near-tie moved this row: the later comparisons hold for the reference's codes only
        assert _rel(lat.cpu(), g["latents"][:, :lat.shape[1]]) < 1e-5, k
        np.testing.assert_allclose(float(cm), float(g[f"cm_{k}"]), rtol=1e-5)
        np.testing.assert_allclose(float(cb), float(g[f"cb_{k}"]), rtol=1e-5)
        if f"z_{k}" in g:
            assert _rel(z.cpu(), g[f"z_{k}"]) < 1e-5, k
        if f"audio_{k}" in g:
            a = m.decode(z).cpu().numpy()
            assert a.shape == g[f"audio_{k}"].shape
            assert a.shape[-1] == int(g["decode_len"][0])
            assert _rel_rms(a, g[f"audio_{k}"]) < 1e-4, (k, _rel_rms(a, g[f"audio_{k}"]))


@pytest.mark.parametrize("name", NAMES)
def test_from_codes_decode_and_forward(name):
    g = load_golden(name)
    m = _model(name)
    codes = torch.from_numpy(g["codes_nall"].astype(np.int64)).cuda()
    zq, zp, c = m.quantizer.from_codes(codes)
    assert tuple(zp.shape) == tuple(g["fc_zp_shape"]) and c is codes
    assert _rel(zq.cpu(), g["fc_z"]) < 1e-5
    a = m.decode(zq).cpu().numpy()
    assert _rel_rms(a, g["audio_nall"]) < 1e-4
    x2 = _x(g["fwd_pcm"])
    out = m(x2)
    assert set(out) == {"audio", "z", "codes", "latents", "vq/commitment_loss", "vq/codebook_loss"}
    assert out["audio"].shape[-1] == g["fwd_pcm"].shape[-1] and tuple(out["z"].shape) == tuple(g["fwd_z_shape"])
    np.testing.assert_array_equal(out["codes"].cpu().numpy(), g["fwd_codes"])
    assert _rel_rms(out["audio"].cpu(), g["fwd_audio"]) < 1e-4
    np.testing.assert_allclose(float(out["vq/commitment_loss"]), float(g["fwd_cm"]), rtol=1e-5)
    with pytest.raises(AssertionError):
        m(x2, sample_rate=44100)


def test_prefix_property_and_argument_errors():
    g = load_golden("dac_tiny")
    m = _model("dac_tiny")
    x = _x(g["pcm"])
    full = m.encode(x, 18)[1]
    for n in (1, 2, 6, 12):
        assert torch.equal(m.encode(x, n)[1], full[:, :n])
    assert torch.equal(m.encode(x, 40)[1], full)
    with pytest.raises(ValueError):
        m.encode(x, 0)
    with pytest.raises(ValueError):
        m.encode(x[..., :100])                          # shorter than the encoder's reach: no frame
    m.train()
    try:
        with pytest.raises(NotImplementedError):
            m.encode(x)
    finally:
        m.eval()


@pytest.mark.parametrize("name", ("dac_syn", "dac_tiny"))
def test_batch_independence(name):
    g = load_golden(name)
    m = _model(name)
    L = g["pcm"].shape[-1]
    clips = np.stack([synth.voiced_clip_int16(f"dac-batch-{i}", L) if i % 2 else synth.noise_clip_int16(f"dac-batch-{i}", L) for i in range(8)])
    xb = _x(clips)
    zb, cb_, *_ = m.encode(xb)
    ab = m.decode(zb)
    for i in (0, 3, 7):
        z1, c1, *_ = m.encode(xb[i:i + 1])
        a1 = m.decode(z1)
        assert torch.equal(c1, cb_[i:i + 1]) and torch.equal(a1, ab[i:i + 1]), i


def test_in_place_parameter_change_is_picked_up():
    from esc.baselines import DAC
    name = "dac_syn"
    g = load_golden(name)
    m = DAC(**_cfg(name))
    m.load_state_dict(_sd(name), strict=True)
    m = m.cuda().eval()
    x = _x(g["pcm"])
    a0 = m(x)["audio"].clone()
    with torch.no_grad():
        m.get_parameter("encoder.block.1.block.0.block.1.weight_g").mul_(1.5)
        m.get_parameter("decoder.model.1.block.0.alpha").add_(0.25)
    out = m(x)
    assert not torch.equal(out["audio"], a0)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    r = du.DacRef(_cfg(name), sd).forward(x.cpu())
    np.testing.assert_array_equal(out["codes"].cpu().numpy(), r["codes"].numpy())
    assert _rel_rms(out["audio"].cpu(), r["audio"]) < 1e-4


def test_device_snake_and_tanh_against_fp64():
    """The kernels' Snake and tanh (escx_dac_test_math) within 2 ulp of fp64 over x in [-20, 20] and alpha in [0.1, 3]."""
    from esc import _native
    lib = _native.load()
    xs = torch.linspace(-20.0, 20.0, 20001, dtype=torch.float32)
    al = torch.linspace(0.1, 3.0, 30, dtype=torch.float32)
    X, A = torch.meshgrid(xs, al, indexing="ij")
    X, A = X.reshape(-1).contiguous(), A.reshape(-1).contiguous()
    xd, ad, out = X.cuda(), A.cuda(), torch.empty(X.numel(), device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _native.check(lib.escx_dac_test_math(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(ad.data_ptr()), ctypes.c_void_p(out.data_ptr()), X.numel(), 0, st))
    x64, a64 = X.double(), A.double()
    inv = 1.0 / (a64 + 1e-9)
    ulp = lambda v: torch.abs(v).clamp_min(2.0 ** -126) * 2.0 ** -23          # noqa: E731
    # the fp32 evaluation rounds alpha * x once before the sine: that input rounding is the formula's, not the kernel's; bound the kernel by the
    # fp64 value of the same formula at the rounded product, within 2 ulp of the result plus 2 ulp of each rounded term
    prod = (A * X).double()
    y_r = x64 + inv * torch.sin(prod) ** 2
    err = (out.cpu().double() - y_r).abs()
    assert bool((err <= 2 * ulp(y_r) + 2 * ulp(inv * torch.sin(prod) ** 2)).all()), float((err / ulp(y_r)).max())
    _native.check(lib.escx_dac_test_math(ctypes.c_void_p(xd.data_ptr()), None, ctypes.c_void_p(out.data_ptr()), X.numel(), 1, st))
    t64 = torch.tanh(x64)
    assert bool(((out.cpu().double() - t64).abs() <= 2 * ulp(t64)).all())


def test_abi_parameter_order_and_uncovered_geometry():
    from esc import _native
    from esc.baselines import DAC
    lib = _native.load()
    m = _model("dac_tiny")
    lib_, hd = m._handle(torch.device("cuda:0"))
    keys = [lib.escx_dac_param_key(hd, i).decode() for i in range(lib.escx_dac_param_count(hd))]
    assert keys == list(load_manifest("dac_tiny"))
    assert lib.escx_dac_param_total(hd) == sum(int(np.prod(s)) for s in load_manifest("dac_tiny").values())
    assert lib.escx_dac_num_frames(hd, 16000) == 50 and lib.escx_dac_output_samples(hd, 50) == 15992
    for name in NAMES:
        mm = _model(name)
        _, h2 = mm._handle(torch.device("cuda:0"))
        for L in range(1, 3 * mm.hop_length + 1):
            want = du.num_frames(_cfg(name), L)
            assert lib.escx_dac_num_frames(h2, L) == mm.num_frames(L) == max(want, 0), (name, L)
        short = next(L for L in range(1, mm.hop_length + 1) if mm.num_frames(L) == 1) - 1
        with pytest.raises(ValueError):
            mm.encode(torch.zeros(1, 1, short, device="cuda"))            # the C entry point refuses it too (escx_dac_encode: INVALID_ARG)
        assert mm.encode(torch.zeros(1, 1, short + 1, device="cuda"))[1].shape[-1] == 1
    bad = DAC(encoder_dim=4, encoder_rates=[2], decoder_dim=8, decoder_rates=[2], n_codebooks=1, codebook_size=4, codebook_dim=16,
              sample_rate=16000).cuda().eval()
    with pytest.raises(NotImplementedError):
        bad.encode(torch.zeros(1, 1, 64, device="cuda"))


@pytest.mark.parametrize("name", ("dac_syn", "dac_tiny"))
def test_snake_placement_is_bitwise_neutral(name):
    """Every per-class Snake placement (escx_dac_set_snake_maps) gives bitwise the outputs of the default."""
    g = load_golden(name)
    m = _model(name)
    x = _x(g["pcm"])
    z0, c0, l0, cm0, _ = m.encode(x)
    a0 = m.decode(z0)
    default = _native_lib().escx_dac_get_snake_maps(m._handle(torch.device("cuda:0"))[1])
    try:
        for mask in (0, 1, 2, 4, 8, 16, 31):
            m.set_snake_maps(mask)
            z, c, lat, cm, _ = m.encode(x)
            assert torch.equal(z, z0) and torch.equal(c, c0) and torch.equal(lat, l0) and torch.equal(cm, cm0), mask
            assert torch.equal(m.decode(z0), a0), mask
        with pytest.raises(ValueError):
            m.set_snake_maps(32)
    finally:
        m.set_snake_maps(default)


def test_from_codes_range_check():
    m = _model("dac_syn")
    codes = torch.zeros(1, 2, 5, dtype=torch.int64, device="cuda")
    codes[0, 1, 3] = m.codebook_size
    with pytest.raises(IndexError):
        m.quantizer.from_codes(codes)
    codes[0, 1, 3] = -1
    with pytest.raises(IndexError):
        m.quantizer.from_codes(codes)


def _native_lib():
    from esc import _native
    return _native.load()


def test_dac_base_at_the_timed_size():
    """36 x 3 s through DAC-Base once, against the restatement on the device: every code exact or attributed to a near-tie."""
    name = "dac_base"
    m = _model(name)
    ref = du.DacRef(_cfg(name), {k: v.cuda() for k, v in _sd(name).items()})
    clips = np.stack([synth.voiced_clip_int16(f"dac-big-{i}", 48000) if i % 2 else synth.noise_clip_int16(f"dac-big-{i}", 48000) for i in range(36)])
    x = _x(clips)
    z, codes, lat, cm, cb = m.encode(x)
    with torch.no_grad():
        ze = ref.encoder(x)
        rz, rc, rl, rcm, rcb, mg = ref.quantize(ze, None, margins=True)
    got, want = codes.cpu().numpy(), rc.cpu().numpy()
    rows = 0
    if not np.array_equal(got, want):
        rows, bad = du.attribute_codes(ref, ze, None, got, want, mg.cpu().numpy())
        assert not bad, bad[:5]
    print(f"DAC-Base 36 x 3 s: {codes.numel()} codes, {rows} rows attributed to near-ties")
    a = m.decode(z)
    with torch.no_grad():
        ra = ref.decoder(z)
    assert _rel_rms(a.cpu(), ra.cpu()) < 1e-4
