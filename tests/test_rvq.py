"""The rvq+swinT codec (RVQCodecs): construction, state_dict layout and argument errors on the CPU; codes, audio, losses, batch independence,
per-clip counts, the stage entry points, C-ABI errors and the flat-parameter refresh on the MI355X, against the real reference's fixtures
(tools/gen_rvq_golden.py) and the CPU restatement of tests/rvq_util.py."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import rvq_util as ru
from conftest import ROOT, load_golden, load_manifest, synth_state
from esc import synth

NAMES = ("rvq_tiny", "rvq_base")


def _cfg(name):
    return json.loads(str(load_golden(name)["config_json"]))


def _rms(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_import_and_make_model():
    import esc
    import esc.models
    from esc import RVQCodecs
    from esc.models import make_model, model_dict
    assert esc.RVQCodecs is RVQCodecs is esc.models.RVQCodecs is model_dict["rvq+swinT"]
    cfg = _cfg("rvq_base")
    m = make_model(cfg, "rvq+swinT")
    assert type(m) is RVQCodecs and m.max_streams == 6 and m.num_rvqs == 6
    assert type(make_model(_cfg("rvq_tiny"), "rvq+swinT")) is RVQCodecs
    d = RVQCodecs()                                           # the reference's defaults (codecs.py:98-121) are the ablation yaml
    assert d.state_dict().keys() == m.state_dict().keys()


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_layout_and_strict_load(name):
    from esc.models import make_model
    man = load_manifest(name)
    m = make_model(_cfg(name), "rvq+swinT")
    got = {k: list(v.shape) for k, v in m.state_dict().items()}
    assert got == man
    assert len(man) == (400 if name == "rvq_base" else 208)
    m.load_state_dict(synth_state(name), strict=True)
    with pytest.raises(RuntimeError):
        m.load_state_dict({k: v for k, v in synth_state(name).items() if "proj_up" not in k}, strict=True)


@pytest.mark.parametrize("name,bps", [("rvq_base", 9.0), ("rvq_tiny", 2.0)])
def test_max_bps(name, bps):
    from esc.models import make_model
    m = make_model(_cfg(name), "rvq+swinT")
    assert m.max_bps == bps == float(load_golden(name)["max_bps"])


def test_argument_errors():
    from esc import RVQCodecs
    m = RVQCodecs(**_cfg("rvq_tiny")).eval()
    x = torch.zeros(2, 1280)
    for bad in (0, -1):
        with pytest.raises(ValueError):
            m.encode(x, bad)
        with pytest.raises(ValueError):
            m(x, None, bad)
    with pytest.raises(ValueError, match="entries"):
        m.encode(x, [1, 2, 3])                                # per-clip counts of the wrong length
    with pytest.raises(ValueError):
        m.encode(x, [1, 5])                                   # above num_rvqs
    with pytest.raises(ValueError, match="entries"):
        m.decode(torch.zeros(2, 4, 3, 16, dtype=torch.int64), (4, 32), num_streams=[1])
    m.train()
    with pytest.raises(NotImplementedError, match="RVQCodecs training is not implemented"):
        m(x, None, 4)
    with pytest.raises(NotImplementedError):
        RVQCodecs(**dict(_cfg("rvq_tiny"), backbone="convolution"))


def test_make_model_names_and_configurations():
    """make_model builds rvq+swinT from a configuration that states its quantiser (the ablation yaml's model section); an empty one and the
    convolution-backbone names raise NotImplementedError (tests/test_abi.py keeps make_model({}, "rvq+swinT") refused)."""
    from esc import RVQCodecs
    from esc.models import make_model
    assert type(make_model(_cfg("rvq_base"), "rvq+swinT")) is RVQCodecs
    assert type(make_model(dict(num_rvqs=6, codebook_dim=8), "rvq+swinT")) is RVQCodecs
    for cfg, name in (({}, "rvq+swinT"), (dict(num_rvqs=6), "rvq+swinT"), ({}, "rvq+conv"), ({}, "csvq+conv")):
        with pytest.raises(NotImplementedError):
            make_model(cfg, name)


@pytest.mark.parametrize("name", NAMES)
def test_restatement_reproduces_the_reference(name):
    orc, g, cfg, _ = ru.load(name)
    x = torch.from_numpy(synth.pcm_to_float(g["pcm"]))
    tok, shape = orc.bottleneck(x)
    assert tuple(shape) == tuple(g["feat_shape"])
    z = orc.project(tok)
    np.testing.assert_allclose(z.numpy(), g["z_proj"], atol=1e-6, rtol=1e-6)
    codes, margins, _ = orc.quantize(z, cfg["num_rvqs"] + 2)                # above num_rvqs: num_rvqs streams
    assert np.array_equal(codes.numpy(), g["codes"].astype(np.int64))
    np.testing.assert_allclose(margins.numpy(), g["margins"], atol=1e-5)
    for s in range(1, cfg["num_rvqs"] + 1):
        c, _, cm = orc.quantize(z, s)
        assert np.array_equal(c.numpy(), g[f"codes_s{s}"].astype(np.int64))
        np.testing.assert_allclose(cm.numpy(), g[f"cm_loss_s{s}"], rtol=1e-5)
        if f"audio_s{s}" in g:
            a = orc.decode(c, shape).numpy()
            ref = g[f"audio_s{s}"]
            got = a if a.shape == ref.shape else a[:, ::8]
            assert _rms(got, ref) <= 1e-6
            np.testing.assert_allclose(np.sqrt((a.astype(np.float64) ** 2).mean(axis=1)), g[f"audio_rms_s{s}"], rtol=1e-5)


def test_parity_rule_helper():
    """attribute(): a flip at a reference near-tie is accepted when the later stages follow the continued restatement, refused otherwise."""
    orc, g, cfg, _ = ru.load("rvq_tiny")
    ref = g["codes"].astype(np.int64)
    z = g["z_proj"]
    assert ru.attribute(orc, ref, ref, g["margins"], z) == []
    got = ref.copy()
    got[0, 0, 1, 3] = (got[0, 0, 1, 3] + 1) % 64
    assert ru.attribute(orc, got, ref, g["margins"], z) == [(0, 1, 3, 0)]          # margins here are far above the near-tie bound
    margins = g["margins"].copy(); margins[0, 0, 1, 3] = 0.0
    cont = [k for k, _ in ru.continue_vector(orc, torch.from_numpy(z[0, 3, 1].copy()), 1, [got[0, 0, 1, 3]])]
    got[0, :, 1, 3] = cont
    assert ru.attribute(orc, got, ref, margins, z) == []
    got[0, -1, 1, 3] = (got[0, -1, 1, 3] + 1) % 64
    assert ru.attribute(orc, got, ref, margins, z) != []


# ---------------------------------------------------------------------------------------------------------------- GPU
def _model(name, precision=None, sd=None):
    from esc.models import make_model
    m = make_model(_cfg(name), "rvq+swinT")
    m.load_state_dict(sd if sd is not None else synth_state(name), strict=True)
    m = m.to("cuda:0").eval()
    if precision is not None:
        m.set_precision(precision)
    return m


@pytest.fixture(scope="module")
def fixtures():
    return {n: ru.load(n) for n in NAMES}


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["f16x2", "bf16x3", "fp32"])
@pytest.mark.parametrize("name", NAMES)
def test_codes_audio_losses_against_the_reference(name, precision, fixtures):
    orc, g, cfg, sd = fixtures[name]
    model = _model(name, precision, sd)
    assert model.precision == precision
    x = torch.from_numpy(synth.pcm_to_float(g["pcm"])).cuda()
    R = cfg["num_rvqs"]
    full, shape = model.encode(x, R + 3)                                      # above num_rvqs: num_rvqs streams, as the reference
    assert tuple(full.shape) == (2, R, cfg["group_size"], g["codes"].shape[-1]) and tuple(shape) == tuple(g["feat_shape"])
    bad = ru.attribute(orc, full.cpu().numpy(), g["codes"].astype(np.int64), g["margins"], g["z_proj"])
    assert bad == [], f"{precision}: unattributable code differences at (b, g, t, stage) {bad[:8]}"
    for s in range(1, R + 1):
        codes, shp = model.encode(x, s)
        assert torch.equal(codes, full[:, :s]), f"S={s}: not a prefix of the num_rvqs-stream codes"
        out = model(x, None, s)
        assert torch.equal(out["codes"], codes)
        audio = model.decode(codes, shp)
        assert torch.equal(out["recon_audio"], audio), f"S={s}: eval forward != decode(encode(x))"
        same = np.array_equal(codes.cpu().numpy(), g[f"codes_s{s}"].astype(np.int64))
        if same:                                                            # a (legal) near-tie flip changes the bottleneck and with it the rest
            np.testing.assert_allclose(out["cm_loss"].cpu().numpy(), g[f"cm_loss_s{s}"], rtol=1e-5)
            np.testing.assert_allclose(out["cb_loss"].cpu().numpy(), g[f"cb_loss_s{s}"], rtol=1e-5)
            if f"audio_s{s}" in g:
                a = audio.cpu().numpy()
                ref = g[f"audio_s{s}"]
                assert _rms(a if a.shape == ref.shape else a[:, ::8], ref) <= 1e-4
        else:
            ref_audio = orc.decode(codes.cpu(), shp).numpy()
            assert _rms(audio.cpu().numpy(), ref_audio) <= 1e-4
    xf = out["raw_feat"]                                                    # forward(x, x_feat): the same outputs from the given spectrum
    out2 = model(x, xf.permute(0, 2, 3, 1).contiguous(), R)
    out1 = model(x, None, R)
    assert torch.equal(out2["codes"], out1["codes"]) and torch.equal(out2["recon_audio"], out1["recon_audio"])


@pytest.mark.gpu
def test_codes_do_not_depend_on_the_batch(fixtures):
    orc, g, cfg, sd = fixtures["rvq_base"]
    model = _model("rvq_base", sd=sd)
    pcm = np.stack([synth.noise_clip_int16(f"rvq-batch-{i}", 48000) if i % 2 else synth.voiced_clip_int16(f"rvq-batch-{i}", 48000)
                    for i in range(288)])
    x = torch.from_numpy(synth.pcm_to_float(pcm)).cuda()
    big, _ = model.encode(x, 6)
    mid, _ = model.encode(x[:36], 6)
    assert torch.equal(big[:36], mid)
    for i in (0, 1, 35, 144, 287):
        one, _ = model.encode(x[i:i + 1], 6)
        assert torch.equal(one[0], big[i]), f"clip {i}"


def _lib_handle(model):
    from esc import _native
    return _native.load(), model._handle(torch.device("cuda:0"))[1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("clustered", [False, True])
def test_stage_entry_points(name, clustered, fixtures):
    """escx_rvq_encode / escx_rvq_decode on deterministic bottleneck tokens against the restatement; the clustered case puts the projected
    vectors between two codebook entries of stage 0, so that many reference margins are below 1e-5."""
    orc, g, cfg, sd = fixtures[name]
    model = _model(name, sd=sd)
    lib, hd = _lib_handle(model)
    from esc import _native
    B, W = 3, 16
    C = cfg["h_dims"][-1]
    gen = torch.Generator().manual_seed(7)
    if not clustered:
        tok = torch.randn((B, orc.Hq * W, C), generator=gen)
    else:                   # frames v with proj_down(v_m) = midpoint of two normalised stage-0 entries (+ a tiny offset): v_m = W^T (W W^T)^-1 z
        T = W // orc.ov
        parts = []
        for m in range(orc.G):
            cbn = torch.nn.functional.normalize(orc.cb(m, 0), dim=-1)
            sim = cbn @ cbn.t() - 3 * torch.eye(cbn.shape[0])
            a = torch.randint(0, cbn.shape[0], (B * T,), generator=gen)
            b = sim[a].argmax(dim=1)                                        # a's nearest neighbour: the midpoint is nearest to both
            zt = (cbn[a] + cbn[b]) / 2 + 2e-6 * torch.randn((B * T, orc.d), generator=gen)
            Wd = sd[f"quantizers.vqs.{m}.proj_down.weight"].double()
            v = (Wd.t() @ torch.linalg.solve(Wd @ Wd.t(), zt.double().t())).t().float()
            parts.append(v.view(B, T, -1))
        tok = ru.pvq_unframes(torch.cat(parts, dim=-1), orc.Hq, orc.ov)
    tok = tok.contiguous()
    z = orc.project(tok)
    R = cfg["num_rvqs"]
    ref, margins, _ = orc.quantize(z, R)
    if clustered:
        assert float((margins[:, 0] < 1e-5).float().mean()) > 0.3, "the clustered tokens should produce many near-ties"
    codes = torch.empty((B, R, orc.G, W // orc.ov), dtype=torch.int64, device="cuda")
    zq = torch.empty((B, orc.Hq * W, C), device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _native.check(lib.escx_rvq_encode(hd, tok.cuda().data_ptr(), B, W, R, codes.data_ptr(), zq.data_ptr(), st))
    torch.cuda.synchronize()
    bad = ru.attribute(orc, codes.cpu().numpy(), ref.numpy(), margins.numpy(), z.numpy(), tol=ru.NEAR_TIE)
    assert bad == [], f"unattributable code differences at (b, g, t, stage) {bad[:8]}"
    got = codes.cpu()
    want = orc.dequantize(got)
    assert _rms(zq.cpu().numpy(), want.numpy()) <= 1e-5 * max(1.0, float(want.abs().max()))
    back = torch.empty_like(zq)
    _native.check(lib.escx_rvq_decode(hd, codes.data_ptr(), B, R, W, back.data_ptr(), st))
    torch.cuda.synchronize()
    assert torch.equal(back, zq), "decode form != the encode form's up-projection"
    two = torch.empty((B, 2, orc.G, W // orc.ov), dtype=torch.int64, device="cuda")
    _native.check(lib.escx_rvq_encode(hd, tok.cuda().data_ptr(), B, W, 2, two.data_ptr(), None, st))
    torch.cuda.synchronize()
    assert torch.equal(two, codes[:, :2])


@pytest.mark.gpu
def test_per_clip_counts_and_esc2(fixtures):
    from esc import bitstream
    orc, g, cfg, sd = fixtures["rvq_tiny"]
    model = _model("rvq_tiny", sd=sd)
    pcm = np.concatenate([g["pcm"], np.stack([synth.noise_clip_int16(f"rvq-mix-{i}", 1280) for i in range(4)])])
    x = torch.from_numpy(synth.pcm_to_float(pcm)).cuda()
    counts = [4, 1, 3, 2, 4, 1]
    codes, shape = model.encode(x, counts)
    out = model(x, None, counts)
    assert torch.equal(out["codes"], codes)
    audio = model.decode(codes, shape, num_streams=counts)
    assert torch.equal(out["recon_audio"], audio)
    for b, s in enumerate(counts):
        u, _ = model.encode(x[b:b + 1], s)
        assert torch.equal(codes[b, :s], u[0]) and bool((codes[b, s:] == -1).all()), f"clip {b}"
        uo = model(x[b:b + 1], None, s)
        assert torch.equal(out["recon_audio"][b], uo["recon_audio"][0]) and torch.equal(out["cm_loss"][b], uo["cm_loss"][0]), f"clip {b}"
        assert torch.equal(audio[b], model.decode(u, shape)[0])
    blob = bitstream.pack_codes(codes, shape, num_streams=counts)
    back, shp, cnt = bitstream.unpack_codes(blob, model=model)
    assert torch.equal(back, codes) and list(cnt) == counts and tuple(shp) == tuple(shape)


@pytest.mark.gpu
def test_c_abi_errors_leave_the_handle_usable(fixtures):
    from esc import _native
    from esc.models import make_model
    orc, g, cfg, sd = fixtures["rvq_tiny"]
    model = _model("rvq_tiny", sd=sd)
    lib, hd = _lib_handle(model)
    assert lib.escx_quantizer_kind(hd) == 1
    esc_model = make_model(json.loads(str(load_golden("tiny")["config_json"])))
    esc_model.load_state_dict(synth_state("tiny"))
    esc_model.to("cuda:0")
    assert lib.escx_quantizer_kind(esc_model._handle(torch.device("cuda:0"))[1]) == 0
    x = torch.from_numpy(synth.pcm_to_float(g["pcm"])).cuda()
    ref, _ = model.encode(x, 4)
    B, L = x.shape
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    codes = torch.empty((B, 6, 3, 16), dtype=torch.int64, device="cuda")
    wave = torch.empty((B, 1260), device="cuda")
    fh, fw = ctypes.c_int(), ctypes.c_int()
    assert lib.escx_encode(hd, x.data_ptr(), B, L, 5, codes.data_ptr(), ctypes.byref(fh), ctypes.byref(fw), st) == _native.ESCX_ERR_INVALID_ARG
    assert lib.escx_encode(hd, x.data_ptr(), B, L, 0, codes.data_ptr(), ctypes.byref(fh), ctypes.byref(fw), st) == _native.ESCX_ERR_INVALID_ARG
    assert lib.escx_decode(hd, codes.data_ptr(), B, 5, 4, 32, wave.data_ptr(), None, st) == _native.ESCX_ERR_INVALID_ARG
    bad = (ctypes.c_int32 * B)(1, 5)
    assert lib.escx_encode_streams(hd, x.data_ptr(), B, L, bad, codes.data_ptr(), None, None, st) == _native.ESCX_ERR_INVALID_ARG
    assert lib.escx_pvq_encode(hd, 0, x.data_ptr(), None, B, 32, codes.data_ptr(), 0, st) == _native.ESCX_ERR_UNSUPPORTED
    assert lib.escx_pvq_decode(hd, 0, codes.data_ptr(), 0, None, B, 32, wave.data_ptr(), st) == _native.ESCX_ERR_UNSUPPORTED
    assert lib.escx_train_forward(hd, None, x.data_ptr(), B, L, 2, 0, codes.data_ptr(), wave.data_ptr(), None, None, None, None, st) == _native.ESCX_ERR_UNSUPPORTED
    assert b"RVQCodecs training" in lib.escx_last_error()
    assert lib.escx_train_backward(hd, None, None, None, None, wave.data_ptr(), st) == _native.ESCX_ERR_UNSUPPORTED
    assert lib.escx_rvq_encode(esc_model._handle(torch.device("cuda:0"))[1], x.data_ptr(), B, 32, 1, codes.data_ptr(), None, st) == _native.ESCX_ERR_UNSUPPORTED
    again, _ = model.encode(x, 4)
    assert torch.equal(again, ref)
    # a geometry the fused kernel does not cover is refused when the handle is created
    odd = make_model(dict(cfg, codebook_dim=6, group_size=2), "rvq+swinT")
    with pytest.raises(NotImplementedError, match="not covered"):
        odd.to("cuda:0").encode(x, 1)


@pytest.mark.gpu
def test_in_place_edits_reach_the_next_call(fixtures):
    """ESC._handle re-packs through the flat-parameter layout after an in-place edit: permuting the rows of a stage-0 codebook permutes its
    codes and leaves every later stage (same raw rows subtracted) and the audio unchanged; scaling proj_up scales the decoder input."""
    orc, g, cfg, sd = fixtures["rvq_tiny"]
    model = _model("rvq_tiny", sd=sd)
    x = torch.from_numpy(synth.pcm_to_float(g["pcm"])).cuda()
    before, shape = model.encode(x, 4)
    audio = model.decode(before, shape)
    K = cfg["codebook_size"]
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(3))
    params = dict(model.named_parameters())
    w = params["quantizers.vqs.0.vqs.0.embedding.weight"]
    with torch.no_grad():
        w.copy_(w.detach().clone()[perm])
    after, _ = model.encode(x, 4)
    inv = torch.argsort(perm).cuda()
    expect = before.clone()
    expect[:, 0, 0] = inv[before[:, 0, 0]]
    assert torch.equal(after, expect)
    assert torch.equal(model.decode(after, shape), audio)
    with torch.no_grad():
        params["quantizers.vqs.1.proj_up.weight"].mul_(0.0)
    assert not torch.equal(model.decode(after, shape), audio)


@pytest.mark.gpu
def test_compress_script_with_an_rvq_config(tmp_path):
    from scipy.io import wavfile
    wav = tmp_path / "in.wav"
    wavfile.write(wav, 16000, synth.voiced_clip_int16("rvq-cli", 48000))
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "efficient-speech-codec_amd"))
    out = subprocess.run([sys.executable, "-m", "scripts.compress", "--input", str(wav), "--save_path", str(tmp_path / "out"), "--synthetic", "rvq_base",
                          "--num_streams", "4", "--device", "cuda"], capture_output=True, text=True, env=env,
                         cwd=os.path.join(ROOT, "efficient-speech-codec_amd"), timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    codes = torch.load(tmp_path / "out" / "encoded_6.0kbps_in.pth")
    assert tuple(codes.shape) == (1, 4, 3, 150)
    from esc import bitstream
    back, _ = bitstream.unpack_codes(open(tmp_path / "out" / "encoded_6.0kbps_in.esc", "rb").read(), device="cuda")
    assert torch.equal(back.cpu(), codes)
