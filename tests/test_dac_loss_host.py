"""CPU-side checks of the DAC baseline's training losses (esc.baselines.loss, include/escx.h escx_spec_loss_*, escx_wave_l1, escx_sisdr): the public surface,
the restatement of tests/dac_loss_util.py against the fixture made from the real reference losses, the dropout rule, and - for EVERY case of the GPU tests
(test_dac_loss.py) - the conditions their bounds rest on, so that a changed seed fails here, on any machine.  If a case fails, change its input, not the bound.
"""
import inspect
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

import dac_loss_util as D
from conftest import GOLDEN, ROOT

NEW_SYMBOLS = ("escx_spec_loss_create", "escx_spec_loss_destroy", "escx_spec_loss_workspace_floats", "escx_spec_loss_eval", "escx_wave_l1", "escx_sisdr")


def test_public_surface():
    import esc.baselines as EB
    from esc import _native
    from esc.baselines import loss as EL
    for name in ("L1Loss", "SISDRLoss", "MultiScaleSTFTLoss", "MelSpectrogramLoss"):
        assert getattr(EB, name) is getattr(EL, name) and name in EB.__all__
    assert EB.DAC is not None and EB.DACFile is not None and "DAC" in EB.__all__ and "DACFile" in EB.__all__
    header = open(os.path.join(ROOT, "include", "escx.h")).read()
    lib = _native.load()
    for sym in NEW_SYMBOLS:
        assert re.search(rf"\b{sym}\s*\(", header), sym
        assert sym in _native.SIGNATURES and hasattr(lib, sym), sym
    assert "escx_spec_loss_config" in header and ctypes_fields(_native.EscxSpecLossConfig) == ["n_scales", "window", "n_mels", "filterbank", "clamp_eps", "pow",
                                                                                                "mag_weight", "log_weight"]


def ctypes_fields(struct):
    return [f[0] for f in struct._fields_]


def test_constructor_defaults_are_the_reference_s():
    """Keywords, their order and their defaults as dac/nn/loss.py:26, 76-83, 174-185, 259-273 (sample_rate is the one addition, last)."""
    from esc.baselines import L1Loss, MelSpectrogramLoss, MultiScaleSTFTLoss, SISDRLoss

    def sig(cls):
        return [(k, p.default) for k, p in inspect.signature(cls.__init__).parameters.items() if k not in ("self", "kwargs")]

    assert sig(L1Loss) == [("attribute", "audio_data"), ("weight", 1.0)]
    assert sig(SISDRLoss) == [("scaling", True), ("reduction", "mean"), ("zero_mean", True), ("clip_min", None), ("weight", 1.0)]
    s = sig(MultiScaleSTFTLoss)
    assert [k for k, _ in s] == ["window_lengths", "loss_fn", "clamp_eps", "mag_weight", "log_weight", "pow", "weight", "match_stride", "window_type", "sample_rate"]
    d = dict(s)
    assert d["window_lengths"] == [2048, 512] and type(d["loss_fn"]) is nn.L1Loss and (d["clamp_eps"], d["mag_weight"], d["log_weight"], d["pow"], d["weight"]) == (1e-5, 1.0, 1.0, 2.0, 1.0)
    assert d["match_stride"] is False and d["window_type"] is None and d["sample_rate"] == 16000
    s = sig(MelSpectrogramLoss)
    assert [k for k, _ in s] == ["n_mels", "window_lengths", "loss_fn", "clamp_eps", "mag_weight", "log_weight", "pow", "weight", "match_stride", "mel_fmin", "mel_fmax",
                                 "window_type", "sample_rate"]
    d = dict(s)
    assert d["n_mels"] == [150, 80] and d["window_lengths"] == [2048, 512] and d["mel_fmin"] == [0.0, 0.0] and d["mel_fmax"] == [None, None]
    assert (d["clamp_eps"], d["mag_weight"], d["log_weight"], d["pow"], d["weight"]) == (1e-5, 1.0, 1.0, 2.0, 1.0)
    m = MelSpectrogramLoss(n_mels=D.YML["n_mels"], window_lengths=D.YML["window_lengths"])
    assert [s[:2] for s in m._scales()] == [(32, 5), (64, 10)]                      # the zip stops at the two default entries of mel_fmin / mel_fmax
    assert L1Loss().reduction == "mean" and L1Loss().attribute == "audio_data" and SISDRLoss().weight == 1.0


def test_refused_arguments_raise():
    from esc.baselines import L1Loss, MelSpectrogramLoss, MultiScaleSTFTLoss, SISDRLoss
    for cls in (MultiScaleSTFTLoss, MelSpectrogramLoss):
        for kw, word in ((dict(loss_fn=nn.MSELoss()), "loss_fn"), (dict(loss_fn=nn.L1Loss(reduction="sum")), "loss_fn"), (dict(match_stride=True), "match_stride"),
                         (dict(window_type="sqrt_hann"), "window_type")):
            with pytest.raises(NotImplementedError, match=word):
                cls(**kw)
        cls(window_type="hann")
    with pytest.raises(NotImplementedError, match="reduction"):
        L1Loss(reduction="none")
    x = torch.zeros(2, 1, 3000)
    for loss in (L1Loss(), SISDRLoss(), MultiScaleSTFTLoss(), MelSpectrogramLoss()):
        with pytest.raises(RuntimeError, match="HIP device"):
            loss(x, x)


def _close(got, want, tag):
    v, a, b = got
    assert abs(float(v) - float(want[0])) <= 1e-6 * abs(float(want[0])), tag
    assert D.rel_rms(a, want[1].astype(np.float64)) <= 1e-6 and D.rel_rms(b, want[2].astype(np.float64)) <= 1e-6, tag


def test_restatement_reproduces_the_reference_fixture():
    """tests/golden/dac_loss.npz was written by the real dac/nn/loss.py in float64: values to 1e-6 relative, gradients to 1e-6 relative RMS."""
    g = np.load(os.path.join(GOLDEN, "dac_loss.npz"))
    est, ref, est_wave = torch.from_numpy(g["est"]), torch.from_numpy(g["ref"]), torch.from_numpy(g["est_wave"])
    assert est.shape == ref.shape == est_wave.shape == (2, 2049) and "NOT PINNED" in str(g["readme"])
    for name, cfg in D.CONFIGS.items():
        _close(D.spec_reference(est, ref, cfg, torch.float64), (g[f"{name}_loss"], g[f"{name}_d_est"], g[f"{name}_d_ref"]), name)
    two = D.with_(D.DEFAULTS, n_mels=[5, 10], window_lengths=[32, 64], name="zip")
    _close(D.spec_reference(est, ref, two, torch.float64), (g["zip_loss"], g["zip_d_est"], g["zip_d_ref"]), "zip")
    _close(D.with_grads(D.wave_l1, est_wave, ref, torch.float64), (g["l1_loss"], g["l1_d_est"], g["l1_d_ref"]), "l1")
    _close(D.with_grads(lambda r, e: D.sisdr(r, e).mean(), ref, est_wave, torch.float64), (g["sisdr_loss"], g["sisdr_d_ref"], g["sisdr_d_est"]), "sisdr")
    for scaling, zero_mean, clip_min in D.SISDR_OPTIONS:
        for reduction in ("mean", "sum"):
            want = float(g[f"sisdr_{int(scaling)}{int(zero_mean)}{'c' if clip_min is not None else 'n'}_{reduction}"])
            got = float(D.reduce(D.sisdr(ref.double(), est_wave.double(), scaling, zero_mean, clip_min), reduction))
            assert abs(got - want) <= 1e-6 * abs(want)
    for name in ("yml", "defaults", "two"):           # ... and the fixture's spectral case is one the device test may hold to the tolerances
        _spec_conditions(est, ref, D.CONFIGS[name], f"fixture {name}")
    _spec_conditions(est, ref, D.STFT, "fixture stft", grads=False)       # margins and value; its gradients are held to the STFT loss's bound on the device


def test_slaney_filterbanks():
    """No empty filter at the seven yml scales (nor in the other configurations); the package's filterbank is the restatement's, bit for bit; area normalisation."""
    from esc.baselines.loss import slaney_filterbank
    for cfg in D.MEL_CONFIGS:
        for w, nm, fmin, fmax in D.scales(cfg):
            fb = D.slaney(w, nm, fmin, fmax)
            assert fb.shape == (nm, w // 2 + 1) and fb.dtype == np.float32 and (fb >= 0).all()
            assert (fb.max(axis=1) > 0).all(), (w, nm)
            assert np.array_equal(slaney_filterbank(D.SR, w, nm, fmin, fmax), fb)
    fb = D.slaney(2048, 320).astype(np.float64)
    assert abs(fb[0].sum() * D.SR / 2048 - 1.0) < 0.05          # norm="slaney": unit area in Hz
    assert abs(float(D._mel_to_hz(D._hz_to_mel(4321.0))) - 4321.0) < 1e-9 and float(D._hz_to_mel(1000.0)) == 15.0


@pytest.mark.parametrize("dropout", [0, 0.5, 1])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_sample_n_quantizers(dropout, B):
    from esc.baselines import DAC
    model = DAC(encoder_dim=8, encoder_rates=[2, 2], decoder_dim=32, decoder_rates=[2, 2], n_codebooks=4, codebook_size=64, codebook_dim=4, quantizer_dropout=dropout)
    got = model.sample_n_quantizers(B, torch.Generator().manual_seed(9))
    draws = torch.randint(1, 5, (B,), generator=torch.Generator().manual_seed(9)).tolist()          # nn/quantize.py:168: one draw per clip
    n = int(B * dropout)
    assert isinstance(got, list) and all(type(v) is int for v in got) and len(got) == B
    assert got[:n] == draws[:n] and got[n:] == [4] * (B - n) and all(1 <= v <= 4 for v in got)
    assert model.sample_n_quantizers(B, torch.Generator().manual_seed(9)) == got
    with pytest.raises(ValueError):
        model.sample_n_quantizers(0)


def _spec_conditions(est, ref, cfg, tag, grads=True):
    lin, log, clamp = D.margins(est, ref, cfg)
    l64, a64, b64 = D.spec_reference(est, ref, cfg, torch.float64)
    l32, a32, b32 = D.spec_reference(est, ref, cfg, torch.float32)
    el, ea, eb = D.rel_err(l32, l64), D.rel_rms(a32, a64), D.rel_rms(b32, b64)
    print(f"[dac-loss-host {tag}] margins lin {lin:.2e} log {log:.2e} clamp {clamp:.2e}   float32 restatement: loss {el:.2e}  d_est {ea:.2e}  d_ref {eb:.2e}")
    assert min(lin, log, clamp) >= D.TIE_MARGIN, f"{tag}: margins {lin:.2e} / {log:.2e} / {clamp:.2e}"
    assert el <= D.LOSS_RTOL, f"{tag}: float32 restatement loss {el:.2e} from float64"
    if grads:
        assert ea <= D.GRAD_TOL and eb <= D.GRAD_TOL, f"{tag}: float32 restatement gradients {ea:.2e} / {eb:.2e} from float64"


@pytest.mark.parametrize("name", [c["name"] for c in D.MEL_CONFIGS])
def test_filterbank_cases_are_well_conditioned(name):
    cfg = D.CONFIGS[name]
    for kind, gain, B, L in D.mel_cases(cfg):
        _spec_conditions(*D.case(kind, gain, B, L, name), cfg, f"{name} {kind} x {gain} B={B} L={L}")
    assert len(D.mel_cases(cfg)) == (24 if name == "two" else 23)


def test_stft_cases_are_well_conditioned():
    """Margins and the value; the float32 restatement's own gradient error is the yardstick of the GPU bound there, not a condition."""
    for kind, gain, B, L in D.STFT_CASES:
        _spec_conditions(*D.case(kind, gain, B, L), D.STFT, f"stft {kind} x {gain} B={B} L={L}", grads=False)


def test_the_other_spectral_cases_are_well_conditioned():
    """The inputs of the side-independence, weights / pow / scales, determinism, silence and at-clamp tests."""
    est, ref = D.case("noise", "up", 2, 2049)
    for base in (D.DEFAULTS, D.STFT):
        for kw in ({}, dict(mag_weight=0.0), dict(log_weight=0.0), dict(pow=1.0), dict(pow=1.5)):
            _spec_conditions(est, ref, D.with_(base, **kw), f"{base['name']} {kw}", grads=base is D.DEFAULTS)
    noise, silent = D.U.noise_clip(2, 2049, 41), D.U.silent_clip(2, 2049)
    for name in ("yml", "defaults", "stft"):
        for e, r, tag in ((silent, noise, "silent estimate"), (noise, silent, "silent reference")):
            _spec_conditions(e, r, D.CONFIGS[name], f"{name} {tag}", grads=name != "stft")
    kind, B, L = D.AT_CLAMP
    for name in ("yml", "defaults"):
        cfg = D.CONFIGS[name]
        for gain in ("half", "up"):
            _spec_conditions(*D.case(kind, gain, B, L), cfg, f"{name} at_clamp x {gain}")
        n_est, _ = D.clamp_straddles(*D.case(kind, "half", B, L), cfg)
        _, n_ref = D.clamp_straddles(*D.case(kind, "up", B, L), cfg)
        print(f"[dac-loss-host {name} at_clamp] cells with only the estimate clamped (x 0.5): {n_est}   only the reference clamped (x 1.7): {n_ref}")
        assert min(n_est, n_ref) >= D.AT_CLAMP_MIN_CELLS


def test_l1_cases_have_their_ties():
    for n in D.L1_SIZES:
        for B in (1, 2):
            est, ref, ties = D.l1_case(B, n)
            assert ties.any(dim=1).all() and torch.equal(est[ties], ref[ties]) and bool((est[~ties] != ref[~ties]).all())
            _, a64, b64 = D.with_grads(D.wave_l1, est, ref, torch.float64)
            assert not a64[ties.numpy()].any() and np.array_equal(a64, -b64) and np.array_equal(np.abs(a64[~ties.numpy()]), np.full(int((~ties).sum()), 1.0 / (B * n)))


@pytest.mark.parametrize("B,L", D.SISDR_SHAPES)
def test_sisdr_cases_are_well_conditioned(B, L):
    """The float32 restatement meets LOSS_RTOL / GRAD_TOL on every option; the last clip of a batch of several is below clip_min = -30, the others above."""
    references, estimates = D.sisdr_case(B, L)
    for scaling, zero_mean, clip_min in D.SISDR_OPTIONS:
        per = D.sisdr(references.double(), estimates.double(), scaling, zero_mean, None).numpy()
        assert (per[:B - 1 if B > 1 else B] > -29.0).all() and (B == 1 or per[B - 1] < -31.0), per
        for reduction in D.REDUCTIONS:
            w = D.sisdr_weights(B) if reduction == "none" else None
            fn = lambda r, e: D.reduce(D.sisdr(r, e, scaling, zero_mean, clip_min), reduction)
            l64, r64, e64 = D.with_grads(fn, references, estimates, torch.float64, w)
            l32, r32, e32 = D.with_grads(fn, references, estimates, torch.float32, w)
            assert D.rel_err(np.reshape(l32, -1), np.reshape(l64, -1)) <= D.LOSS_RTOL
            assert D.rel_rms(r32, r64) <= D.GRAD_TOL and D.rel_rms(e32, e64) <= D.GRAD_TOL
