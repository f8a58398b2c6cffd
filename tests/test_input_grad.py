"""Input gradients of the training-mode forward (ESC inside a larger autograd graph) and of the generator losses' raw side.

Fixture: tests/golden/input_grad.npz = the REAL reference's training-mode forward with x (or x_feat) requiring grad, its own loss classes and
loss.mean().backward() (tools/gen_input_grad_golden.py): x.grad / x_feat.grad, codes and per-clip losses.  As in tests/test_train.py, the
trainer-loss gradients are held to the fp32 noise floor of the reference restatement (fp32 vs fp64 oracle), the smooth probe to 1e-4."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import load_golden, synth_state
from esc import synth

LOSS_RTOL = 1e-5
GRAD_TOL = 1e-4


def _fixture():
    return load_golden("input_grad")


def _cfg(g, name):
    return json.loads(str(g[f"{name}_config_json"]))


def _weights(g):
    return json.loads(str(g["weights_json"]))


def _clips(g, name):
    tags = json.loads(str(g[f"{name}_tags"]))
    n = json.loads(str(g["n_samples_json"]))[name]
    pcm = np.stack([synth.noise_clip_int16(tags[0], n), synth.voiced_clip_int16(tags[1], n)])
    return torch.from_numpy(synth.pcm_to_float(pcm))


def _cases(g):
    return [tuple(c) for c in json.loads(str(g["cases_json"]))]


def _rel_rms(a, b, floor=1e-30):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(float(np.sqrt(np.mean(b ** 2))), floor))


def _stft64(x, cfg):
    """The codec's front end in float64 (torch.stft center=True, reflect; oracle.esc_oracle.spec_transform): (B, 2, F, T)."""
    from oracle import esc_oracle as O
    return O.spec_transform(x, O.full_config(cfg))


def _oracle_input_grad(g, name, kind, S, freeze, x, dtype=torch.float64, smooth=None, x_feat=None):
    """The oracle's autograd with the parameters as constants and the input (x, or x_feat (B, F, T, 2)) a leaf.  smooth = (A, R, Q, wc, wb):
    mean_b[wc*cm + wb*cb + <recon_audio, A> + <recon_feat, R> + <raw_feat, Q>] instead of the trainer's losses."""
    from oracle import esc_oracle as O
    sd = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in synth_state(name).items()}
    orc = O.EscOracle(_cfg(g, name), sd, keep_graph=True)
    if kind == "x":
        leaf = x.to(dtype).clone().requires_grad_(True)
        out = orc.forward_train(leaf, S, freeze)
    else:
        leaf = x_feat.to(dtype).clone().requires_grad_(True)
        real = O.spec_transform
        O.spec_transform = lambda _x, _c, _w=None: leaf.permute(0, 3, 1, 2)          # codecs.py:33-34: the given spectrum replaces the STFT
        try:
            out = orc.forward_train(x.to(dtype), S, freeze)
        finally:
            O.spec_transform = real
    if smooth is None:
        ls = O.training_loss(out, _weights(g))
    else:
        A, R, Q, wc, wb = smooth
        total = out["cm_loss"] * wc + out["cb_loss"] * wb + (out["recon_audio"] * A.to(dtype)).sum(1) + (out["recon_feat"] * R.to(dtype)).sum((1, 2, 3)) \
            + (out["raw_feat"] * Q.to(dtype)).sum((1, 2, 3))
        ls = {"loss": total, "scalar": total.mean()}
    ls["scalar"].backward()
    return out, ls, leaf.grad.detach()


def _ref_spec(g, tag):
    """x_feat of a spectrum case: the reference's own STFT of x laid out (B, F, T, 2), as stored by the fixture's generator."""
    return torch.from_numpy(g[f"{tag}_xfeat"])


def _noise_floor(g, name, kind, S, freeze, x, x_feat=None):
    """Relative RMS distance of the fp32 oracle's input gradient from the fp64 one: how well any fp32 evaluation determines it."""
    _, _, g64 = _oracle_input_grad(g, name, kind, S, freeze, x, x_feat=x_feat)
    _, _, g32 = _oracle_input_grad(g, name, kind, S, freeze, x, dtype=torch.float32, x_feat=x_feat)
    return g64, _rel_rms(g32.numpy(), g64.numpy())


# ------------------------------------------------------------------------------------------------ CPU: the oracle is pinned
def test_oracle_input_grad_matches_reference():
    """The oracle's autograd reproduces the reference's x.grad / x_feat.grad within the measured fp32 noise floor (fp32 oracle vs fp64)."""
    g = _fixture()
    for kind, name, S, freeze in _cases(g):
        x = _clips(g, name)
        tag = f"{kind}_{name}_s{S}_f{int(freeze)}"
        xf = _ref_spec(g, tag) if kind == "feat" else None
        out, ls, g32 = _oracle_input_grad(g, name, kind, S, freeze, x, dtype=torch.float32, x_feat=xf)
        assert np.array_equal(out["codes"].numpy(), g[f"{tag}_codes"].astype(np.int64)), f"{tag}: codes differ from the reference"
        np.testing.assert_allclose(ls["loss"].detach().numpy(), g[f"{tag}_loss"], rtol=LOSS_RTOL, atol=1e-7, err_msg=tag)
        g64, floor = _noise_floor(g, name, kind, S, freeze, x, x_feat=xf)
        err = _rel_rms(g32.numpy(), g[f"{tag}_grad"])
        err64 = _rel_rms(g[f"{tag}_grad"], g64.numpy())
        print(f"[{tag}] oracle fp32 vs reference {err:.2e}; reference vs fp64 {err64:.2e}; fp32 noise floor {floor:.2e}")
        assert err <= 4 * floor + 1e-6, f"{tag}: oracle vs reference input gradient rel rms {err:.3e} (noise floor {floor:.3e})"
        assert err64 <= 4 * floor + 1e-6, f"{tag}: reference vs fp64 oracle {err64:.3e} (noise floor {floor:.3e})"


def test_fixture_is_small_and_complete():
    g = _fixture()
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "input_grad.npz")) < 512 * 1024
    kinds = {c[0] for c in _cases(g)}
    assert kinds == {"x", "feat"}
    assert any(c[3] for c in _cases(g)) and any(not c[3] and c[2] < _cfg(g, c[1])["max_streams"] for c in _cases(g))


# ------------------------------------------------------------------------------------------------ GPU: the HIP backward
def _model(g, name, frozen=False):
    from esc.models import make_model
    model = make_model(_cfg(g, name))
    model.load_state_dict(synth_state(name))
    model = model.cuda().train()
    if frozen:
        model.requires_grad_(False)
    return model


def _product(model, g, kind, S, freeze, x, smooth=None, x_feat=None):
    """One training step of esc.ESC with the input as a leaf; returns (out, per-clip loss, input grad)."""
    from esc.modules import ComplexSTFTLoss, MelSpectrogramLoss
    if kind == "x":
        leaf = x.cuda().clone().requires_grad_(True)
        out = model(x=leaf, x_feat=None, num_streams=S, freeze_codebook=freeze)
    else:
        leaf = x_feat.cuda().clone().requires_grad_(True)
        out = model(x=x.cuda(), x_feat=leaf, num_streams=S, freeze_codebook=freeze)
    if smooth is None:
        w = _weights(g)
        mel = MelSpectrogramLoss()(out["raw_audio"], out["recon_audio"])
        stft = ComplexSTFTLoss()(out["raw_feat"], out["recon_feat"])
        loss = out["cm_loss"] * w["cm_weight"] + out["cb_loss"] * w["cb_weight"] + mel * w["mel_weight"] + stft * w["stft_weight"]
    else:
        A, R, Q, wc, wb = smooth
        loss = out["cm_loss"] * wc + out["cb_loss"] * wb + (out["recon_audio"] * A.cuda()).sum(1) + (out["recon_feat"] * R.cuda()).sum((1, 2, 3)) \
            + (out["raw_feat"] * Q.cuda()).sum((1, 2, 3))
    loss.mean().backward()
    torch.cuda.synchronize()
    return out, loss.detach().cpu(), (leaf.grad.detach().cpu() if leaf.grad is not None else None)


def _smooth_probe(g, name, x, seed=77):
    cfg = _cfg(g, name)
    gen = torch.Generator().manual_seed(seed)
    hop = int(cfg["hop_len"] * cfg["sr"] * 1e-3)
    T = 1 + x.shape[1] // hop
    A = torch.randn(x.shape, generator=gen) / x.shape[1]
    R = torch.randn(x.shape[0], 2, cfg["in_freq"], (T // 2) * 2, generator=gen) / (cfg["in_freq"] * T)
    Q = torch.randn(x.shape[0], 2, cfg["in_freq"], T, generator=gen) / (cfg["in_freq"] * T)
    return A, R, Q, 0.7, 1.3


@pytest.mark.gpu
def test_input_grad_against_fixture_and_fp64_oracle():
    """x.grad and x_feat.grad of the HIP backward: the smooth probe within 1e-4 of the fp64 oracle, the trainer's losses within the fp32 noise
    floor of the fp64 oracle and of the reference fixture.  Codes are compared first."""
    g = _fixture()
    for kind, name, S, freeze in _cases(g):
        tag = f"{kind}_{name}_s{S}_f{int(freeze)}"
        x = _clips(g, name)
        xf = _ref_spec(g, tag) if kind == "feat" else None
        model = _model(g, name)
        out, loss, gx = _product(model, g, kind, S, freeze, x, x_feat=xf)
        assert np.array_equal(out["codes"].cpu().numpy(), g[f"{tag}_codes"].astype(np.int64)), f"{tag}: codes differ from the reference"
        assert gx is not None, f"{tag}: no input gradient"
        np.testing.assert_allclose(loss.numpy(), g[f"{tag}_loss"], rtol=LOSS_RTOL, atol=1e-7, err_msg=tag)
        g64, floor = _noise_floor(g, name, kind, S, freeze, x, x_feat=xf)
        err64, errf = _rel_rms(gx.numpy(), g64.numpy()), _rel_rms(gx.numpy(), g[f"{tag}_grad"])
        print(f"[{tag}] HIP vs fp64 {err64:.2e}, vs reference {errf:.2e}; fp32 noise floor {floor:.2e}")
        assert err64 <= 4 * floor + 1e-5, f"{tag}: input gradient vs fp64 oracle rel rms {err64:.3e} (noise floor {floor:.3e})"
        assert errf <= 8 * floor + 1e-5, f"{tag}: input gradient vs reference rel rms {errf:.3e} (noise floor {floor:.3e})"
        probe = _smooth_probe(g, name, x)
        model = _model(g, name)
        out, loss, gx = _product(model, g, kind, S, freeze, x, smooth=probe, x_feat=xf)
        oout, ols, g64 = _oracle_input_grad(g, name, kind, S, freeze, x, smooth=probe, x_feat=xf)
        assert torch.equal(out["codes"].cpu(), oout["codes"])
        err = _rel_rms(gx.numpy(), g64.numpy())
        print(f"[{tag} smooth] HIP vs fp64 {err:.2e}")
        assert err <= GRAD_TOL, f"{tag} smooth probe: input gradient rel rms {err:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("L", [167, 259, 1280])
def test_stft_adjoint_alone(L):
    """A cotangent on raw_feat only: x.grad is the adjoint of the codec's STFT (center=True, reflect), equal to torch autograd of torch.stft in
    float64.  Odd frame counts (T = 9, 13, 65) and clips just above the reflect-padding minimum."""
    g = _fixture()
    cfg = _cfg(g, "tiny")
    x = torch.from_numpy(synth.pcm_to_float(np.stack([synth.noise_clip_int16(f"stft-adj-{L}-{i}", L) for i in range(2)])))
    model = _model(g, "tiny", frozen=True)
    leaf = x.cuda().clone().requires_grad_(True)
    out = model(x=leaf, x_feat=None, num_streams=3, freeze_codebook=False)
    T = out["raw_feat"].shape[-1]
    assert T % 2 == 1
    Q = torch.randn(out["raw_feat"].shape, generator=torch.Generator().manual_seed(L), dtype=torch.float64)
    (out["raw_feat"] * Q.float().cuda()).sum().backward()
    x64 = x.double().requires_grad_(True)
    (_stft64(x64, cfg) * Q).sum().backward()
    err = _rel_rms(leaf.grad.cpu().numpy(), x64.grad.numpy())
    print(f"[L={L} T={T}] STFT adjoint rel rms {err:.2e}")
    assert err <= 2e-6, err


@pytest.mark.gpu
def test_wave_grad_is_stft_adjoint_of_spectrum_grad():
    """x.grad equals the STFT adjoint of x_feat.grad taken at x_feat = STFT(x) (the raw-path term rides in both)."""
    g = _fixture()
    name = "tiny"
    x = _clips(g, name)
    probe = _smooth_probe(g, name, x, seed=5)
    out_x, _, gx = _product(_model(g, name), g, "x", 2, False, x, smooth=probe)
    xf = out_x["raw_feat"].detach().permute(0, 2, 3, 1).contiguous().cpu()          # (B, 2, F, T) -> (B, F, T, 2)
    out_f, _, gf = _product(_model(g, name), g, "feat", 2, False, x, smooth=probe, x_feat=xf)
    assert torch.equal(out_x["codes"], out_f["codes"])
    x64 = x.double().requires_grad_(True)
    (_stft64(x64, _cfg(g, name)) * gf.double().permute(0, 3, 1, 2)).sum().backward()
    err = _rel_rms(gx.numpy(), x64.grad.numpy())
    print(f"x.grad vs STFT adjoint of x_feat.grad: rel rms {err:.2e}")
    assert err <= 1e-5, err


@pytest.mark.gpu
def test_loss_modules_raw_side_gradients():
    """ComplexSTFTLoss / MelSpectrogramLoss: the raw-side gradient matches the oracle's autograd; the recon-side gradient is bitwise the same
    whether or not the raw side is requested."""
    from oracle import esc_oracle as O
    from esc.modules import ComplexSTFTLoss, MelSpectrogramLoss
    gen = torch.Generator().manual_seed(11)
    raw, rec = torch.randn(2, 2, 48, 64, generator=gen), torch.randn(2, 2, 48, 64, generator=gen)
    for want_raw in (False, True):
        r = raw.cuda().requires_grad_(want_raw)
        y = rec.cuda().requires_grad_(True)
        ComplexSTFTLoss()(r, y).sum().backward()
        if want_raw:
            r64 = raw.double().requires_grad_(True)
            O.complex_stft_loss(r64, rec.double()).sum().backward()
            assert _rel_rms(r.grad.cpu().numpy(), r64.grad.numpy()) <= GRAD_TOL
            assert torch.equal(y.grad, y_plain)
        else:
            assert r.grad is None
            y_plain = y.grad.clone()
    wav = torch.from_numpy(synth.pcm_to_float(np.stack([synth.voiced_clip_int16("mel-raw-0", 4000), synth.noise_clip_int16("mel-raw-1", 4000)])))
    rec_w = wav * 0.7 + 0.01 * torch.randn(wav.shape, generator=gen)
    for want_raw in (False, True):
        r = wav.cuda().requires_grad_(want_raw)
        y = rec_w.cuda().requires_grad_(True)
        MelSpectrogramLoss()(r, y).sum().backward()
        if want_raw:
            r64 = wav.double().requires_grad_(True)
            O.mel_spectrogram_loss(r64, rec_w.double()).sum().backward()
            err = _rel_rms(r.grad.cpu().numpy(), r64.grad.numpy())
            print(f"mel loss raw-side gradient rel rms {err:.2e}")
            assert err <= GRAD_TOL, err
            assert torch.equal(y.grad, y_plain)
        else:
            y_plain = y.grad.clone()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "base"])
def test_frozen_codec_input_only_backward(name):
    """requires_grad_(False): x.grad is bitwise the full backward's, no p.grad is written, and no parameter-gradient launch runs (profiling on,
    which also forces one batch part: no B.dw_* label in the report).  Base covers the fused MLP backward of the wide token maps."""
    from esc import _native
    g = _fixture()
    x = _clips(g, name)
    _, _, full = _product(_model(g, name), g, "x", 2, False, x)
    model = _model(g, name, frozen=True)
    lib, hd = model._handle(torch.device("cuda", 0), for_training=True)
    _native.check(lib.escx_profile_enable(hd, 1))
    try:
        _, _, only = _product(model, g, "x", 2, False, x)
        report = (lib.escx_profile_report(hd) or b"").decode()
    finally:
        _native.check(lib.escx_profile_enable(hd, 0))
    assert torch.equal(only, full), "input-only backward differs from the full backward's input gradient"
    assert all(p.grad is None for p in model.parameters())
    assert "B.dx_patch" in report and "B.stft_adjoint" in report, report
    assert "B.dw_" not in report, report


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["x", "feat"])
def test_parameter_gradients_unchanged_by_input_grad(kind):
    """Parameter gradients are bitwise the same with and without the input requiring grad."""
    from esc.modules import ComplexSTFTLoss, MelSpectrogramLoss
    g = _fixture()
    x = _clips(g, "tiny")
    xf = _ref_spec(g, "feat_tiny_s2_f0").cuda() if kind == "feat" else None
    grads = []
    for want in (False, True):
        model = _model(g, "tiny")
        inp = (xf if kind == "feat" else x.cuda()).clone().requires_grad_(want)
        out = model(x=x.cuda() if kind == "feat" else inp, x_feat=inp if kind == "feat" else None, num_streams=2, freeze_codebook=False)
        loss = MelSpectrogramLoss()(out["raw_audio"], out["recon_audio"]) + ComplexSTFTLoss()(out["raw_feat"], out["recon_feat"]) + out["cm_loss"]
        loss.mean().backward()
        assert (inp.grad is not None) == want
        grads.append({k: p.grad.clone() for k, p in model.named_parameters()})
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k


@pytest.mark.gpu
def test_multi_part_batch_input_grad(monkeypatch):
    """A batch of 8 splits into parts in the backward; each clip's x.grad matches the one-part run (ESCX_TRAIN_PARTS=1, read per call)."""
    g = _fixture()
    n = json.loads(str(g["n_samples_json"]))["tiny"]
    x = torch.from_numpy(synth.pcm_to_float(np.stack([(synth.voiced_clip_int16 if i % 2 else synth.noise_clip_int16)(f"input-grad-parts-{i}", n)
                                                      for i in range(8)])))
    probe = _smooth_probe(g, "tiny", x, seed=3)
    res = []
    for parts in ("2", "1"):
        monkeypatch.setenv("ESCX_TRAIN_PARTS", parts)
        res.append(_product(_model(g, "tiny"), g, "x", 3, False, x, smooth=probe))
    assert torch.equal(res[0][0]["codes"], res[1][0]["codes"])
    for b in range(8):
        err = _rel_rms(res[0][2][b].numpy(), res[1][2][b].numpy())
        assert err <= 1e-5, f"clip {b}: {err:.3e}"


@pytest.mark.gpu
def test_train_backward_ex_errors():
    """escx_train_backward_ex: both outputs NULL -> ESCX_ERR_INVALID_ARG; an RVQCodecs handle -> ESCX_ERR_UNSUPPORTED; an input gradient
    before any training forward -> ESCX_ERR_STATE."""
    from esc import _native
    from esc.models import make_model
    g = _fixture()
    lib = _native.load()
    for name in ("escx_train_backward_ex", "escx_stft_loss_ex", "escx_mel_loss_ex"):
        assert hasattr(lib, name)
    model = _model(g, "tiny")
    lib, hd = model._handle(torch.device("cuda", 0), for_training=True)
    d_in = torch.empty(2, 1260, device="cuda")
    assert lib.escx_train_backward_ex(hd, None, None, None, None, None, None, ctypes.c_void_p(d_in.data_ptr()), None) == _native.ESCX_ERR_STATE
    out = model(x=_clips(g, "tiny").cuda(), x_feat=None, num_streams=2, freeze_codebook=False)
    assert lib.escx_train_backward_ex(hd, None, None, None, None, None, None, None, None) == _native.ESCX_ERR_INVALID_ARG
    out["recon_audio"].sum().backward()                      # the tape is consumed as usual
    rg = load_golden("rvq_tiny")
    rvq = make_model(json.loads(str(rg["config_json"])), "rvq+swinT")
    rvq.load_state_dict(synth_state("rvq_tiny"))
    rvq = rvq.cuda()
    rhd = rvq._handle(torch.device("cuda", 0))[1]
    assert lib.escx_train_backward_ex(rhd, None, None, None, None, None, None, ctypes.c_void_p(d_in.data_ptr()), None) == _native.ESCX_ERR_UNSUPPORTED
