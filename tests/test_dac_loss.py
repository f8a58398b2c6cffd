"""The training losses of the DAC baseline on the MI355X (esc.baselines.loss; include/escx.h escx_spec_loss_eval, escx_wave_l1, escx_sisdr) against the
float64 restatement of tests/dac_loss_util.py.  test_dac_loss_host.py asserts, on the host, the conditions these bounds rest on for every case used here.

Bounds: values within LOSS_RTOL, gradients within GRAD_TOL relative RMS of float64.  The STFT loss (no filterbank) is the exception the float32 reference
itself is: its own float32 gradient is 4e-6 .. 2e-4 from float64 (near-empty bins, 1 / |S|), so there each gradient must be within
max(GRAD_TOL, 2 x the float32 restatement's error on the same case) - measured against the restatement, never against the device."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import dac_encode_grad_util as eu
import dac_loss_util as D
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _module(cfg, **kw):
    from esc.baselines import MelSpectrogramLoss, MultiScaleSTFTLoss
    k = D.module_kwargs(D.with_(cfg, **kw))
    return (MultiScaleSTFTLoss if cfg["n_mels"] is None else MelSpectrogramLoss)(**k)


def _run(loss, est, ref, need_est=True, need_ref=True, args=None):
    """(value float, d_est, d_ref) of loss(est, ref) on the device; a side that does not require a gradient gives None."""
    a = est.to(DEV).requires_grad_(need_est)
    b = ref.to(DEV).requires_grad_(need_ref)
    v = loss(*(args(a, b) if args else (a, b)))
    if need_est or need_ref:
        v.backward()
    torch.cuda.synchronize()
    g = lambda t: None if t.grad is None else t.grad.detach().cpu().double().numpy()
    return float(v.detach()), g(a), g(b)


def _all_mel_cases():
    return [(cfg["name"],) + c for cfg in D.MEL_CONFIGS for c in D.mel_cases(cfg)]


@pytest.mark.parametrize("name,kind,gain,B,L", _all_mel_cases())
def test_filterbank_losses_against_float64(name, kind, gain, B, L):
    cfg = D.CONFIGS[name]
    est, ref = D.case(kind, gain, B, L, name)
    l64, a64, b64 = D.spec_reference(est, ref, cfg, torch.float64, key=(kind, gain, B, L, D.RESEED.get((name, kind, gain, B, L))))
    v, ga, gb = _run(_module(cfg), est, ref)
    el, ea, eb = D.rel_err([v], [float(l64)]), D.rel_rms(ga, a64), D.rel_rms(gb, b64)
    print(f"[dac-loss {name} {kind} x {gain} B={B} L={L}] loss {el:.2e}  d_est {ea:.2e}  d_ref {eb:.2e}")
    assert el <= D.LOSS_RTOL
    assert ea <= D.GRAD_TOL and eb <= D.GRAD_TOL


@pytest.mark.parametrize("name", [c["name"] for c in D.MEL_CONFIGS] + ["stft"])
def test_gradient_sides_are_independent(name):
    """The reference side gets a gradient only when it requires one; leaving a side out launches nothing for it and does not change the other side's bits."""
    cfg = D.CONFIGS[name]
    est, ref = D.case("noise", "up", 2, 2049)
    loss = _module(cfg)
    v, ga, gb = _run(loss, est, ref)
    v1, ga1, gb1 = _run(loss, est, ref, need_ref=False)
    v2, ga2, gb2 = _run(loss, est, ref, need_est=False)
    v3, ga3, gb3 = _run(loss, est, ref, need_est=False, need_ref=False)
    assert gb1 is None and ga2 is None and ga3 is None and gb3 is None
    assert v == v1 == v2 == v3
    assert np.array_equal(ga, ga1) and np.array_equal(gb, gb2)


@pytest.mark.parametrize("kind,gain,B,L", D.STFT_CASES)
def test_stft_loss_against_float64(kind, gain, B, L):
    cfg = D.STFT
    est, ref = D.case(kind, gain, B, L)
    l64, a64, b64 = D.spec_reference(est, ref, cfg, torch.float64, key=(kind, gain, B, L))
    _, a32, b32 = D.spec_reference(est, ref, cfg, torch.float32, key=(kind, gain, B, L))
    v, ga, gb = _run(_module(cfg), est, ref)
    el, ea, eb = D.rel_err([v], [float(l64)]), D.rel_rms(ga, a64), D.rel_rms(gb, b64)
    ra, rb = D.rel_rms(a32, a64), D.rel_rms(b32, b64)
    print(f"[dac-loss stft {kind} x {gain} B={B} L={L}] loss {el:.2e}  d_est {ea:.2e} (float32 restatement {ra:.2e}, ratio {ea / ra:.2f})  "
          f"d_ref {eb:.2e} (float32 restatement {rb:.2e}, ratio {eb / rb:.2f})")
    assert el <= D.LOSS_RTOL
    assert ea <= max(D.GRAD_TOL, 2 * ra) and eb <= max(D.GRAD_TOL, 2 * rb)


@pytest.mark.parametrize("name", ["yml", "defaults", "stft"])
def test_silence_against_noise(name):
    """A silent estimate against noise and the reverse: finite values at LOSS_RTOL, and exactly zero gradient on the silent side (|S| = 0 everywhere)."""
    cfg = D.CONFIGS[name]
    noise, silent = D.U.noise_clip(2, 2049, 41), D.U.silent_clip(2, 2049)
    for est, ref, zero in ((silent, noise, 0), (noise, silent, 1)):
        l64, a64, b64 = D.spec_reference(est, ref, cfg, torch.float64)
        v, ga, gb = _run(_module(cfg), est, ref)
        assert np.isfinite(v) and np.isfinite(ga).all() and np.isfinite(gb).all()
        assert D.rel_err([v], [float(l64)]) <= D.LOSS_RTOL
        assert not (ga, gb)[zero].any() and not (a64, b64)[zero].any()
        live, ref64 = (ga, gb)[1 - zero], (a64, b64)[1 - zero]
        if name != "stft":
            assert D.rel_rms(live, ref64) <= D.GRAD_TOL
        else:
            r32 = D.spec_reference(est, ref, cfg, torch.float32)[2 - zero]
            assert D.rel_rms(live, ref64) <= max(D.GRAD_TOL, 2 * D.rel_rms(r32, ref64))


@pytest.mark.parametrize("name", ["yml", "defaults"])
@pytest.mark.parametrize("gain", ["half", "up"])
def test_at_clamp_clip(name, gain):
    """Mel cells on both sides of clamp_eps: where the `v >= clamp_eps` branches decide the gradient."""
    cfg = D.CONFIGS[name]
    kind, B, L = D.AT_CLAMP
    est, ref = D.case(kind, gain, B, L)
    l64, a64, b64 = D.spec_reference(est, ref, cfg, torch.float64, key=(kind, gain, B, L))
    v, ga, gb = _run(_module(cfg), est, ref)
    assert D.rel_err([v], [float(l64)]) <= D.LOSS_RTOL
    assert D.rel_rms(ga, a64) <= D.GRAD_TOL and D.rel_rms(gb, b64) <= D.GRAD_TOL


def test_weights_pow_and_scales():
    """mag_weight = 0 and log_weight = 0 each equal the other term alone (their sum the whole); pow 1 against 2; one two-scale handle against the sum of two
    single-scale handles - all against float64, and the decompositions among the device values themselves."""
    est, ref = D.case("noise", "up", 2, 2049)
    for base in (D.DEFAULTS, D.STFT):
        vals = {}
        for tag, kw in (("both", {}), ("log", dict(mag_weight=0.0)), ("mag", dict(log_weight=0.0)), ("pow1", dict(pow=1.0)), ("pow15", dict(pow=1.5))):
            cfg = D.with_(base, **kw)
            l64, a64, _ = D.spec_reference(est, ref, cfg, torch.float64)
            v, ga, _ = _run(_module(base, **kw), est, ref, need_ref=False)
            assert D.rel_err([v], [float(l64)]) <= D.LOSS_RTOL, (base["name"], tag)
            if base is D.DEFAULTS:
                assert D.rel_rms(ga, a64) <= D.GRAD_TOL, (base["name"], tag)
            vals[tag] = (v, ga)
        assert abs(vals["log"][0] + vals["mag"][0] - vals["both"][0]) <= 4 * D.LOSS_RTOL * abs(vals["both"][0])
        assert D.rel_rms(vals["log"][1] + vals["mag"][1], vals["both"][1]) <= 1e-5
        assert vals["pow1"][0] != vals["both"][0]
        wins = base["window_lengths"]
        singles = []
        for i in range(2):
            kw = dict(window_lengths=[wins[i]])
            if base["n_mels"] is not None:
                kw.update(n_mels=[base["n_mels"][i]], mel_fmin=[0.0], mel_fmax=[None])
            singles.append(_run(_module(base, **kw), est, ref, need_ref=False))
        assert abs(singles[0][0] + singles[1][0] - vals["both"][0]) <= 4 * D.LOSS_RTOL * abs(vals["both"][0])
        assert D.rel_rms(singles[0][1] + singles[1][1], vals["both"][1]) <= 1e-5


def test_zip_truncation_and_audio_signal_objects():
    """Seven windows with the two default entries of mel_fmin / mel_fmax are two scales, as in the reference; (B, 1, L) tensors and objects with .audio_data are accepted."""
    from esc.baselines import MelSpectrogramLoss

    class Signal:
        def __init__(self, audio_data):
            self.audio_data = audio_data

    est, ref = D.case("noise", "half", 2, 2049)
    long = MelSpectrogramLoss(n_mels=D.YML["n_mels"], window_lengths=D.YML["window_lengths"])
    short = MelSpectrogramLoss(n_mels=[5, 10], window_lengths=[32, 64])
    v, ga, _ = _run(long, est, ref, need_ref=False)
    v2, ga2, _ = _run(short, est, ref, need_ref=False)
    assert v == v2 and np.array_equal(ga, ga2)
    v3, ga3, _ = _run(short, est.unsqueeze(1), ref.unsqueeze(1), need_ref=False, args=lambda a, b: (Signal(a), Signal(b)))
    assert v3 == v and ga3.shape == (2, 1, 2049) and np.array_equal(ga3[:, 0], ga)
    with pytest.raises(ValueError):
        _module(D.STFT)(torch.zeros(1, 1024, device=DEV), torch.zeros(1, 1024, device=DEV))
    with pytest.raises(RuntimeError):
        short(est, ref)                                   # CPU tensors


def test_determinism_scratch_reuse_and_a_second_handle():
    """Two calls are bitwise equal; a larger call in between (the scratch grows and is reused) and a second handle with another configuration alive at the same
    time do not change the first handle's bits."""
    est, ref = D.case("noise", "step", 2, 2049)
    big_e, big_r = D.case("noise", "up", 3, 4100)
    for cfg, other in ((D.YML, D.DEFAULTS), (D.STFT, D.TWO)):
        loss = _module(cfg)
        first = _run(loss, est, ref)
        again = _run(loss, est, ref)
        _run(loss, big_e, big_r)
        second = _module(other)
        _run(second, big_e, big_r)
        after = _run(loss, est, ref)
        _run(second, est, ref)
        for got in (again, after, _run(loss, est, ref)):
            assert got[0] == first[0] and np.array_equal(got[1], first[1]) and np.array_equal(got[2], first[2])


def test_fp32_spectrum_knob(monkeypatch):
    """The debugging knob of include/escx.h: ESCX_SPEC_LOSS_F32=1 when a handle is created makes that handle compute the STFT loss's spectra with the fp32
    framing GEMM - the value stays within LOSS_RTOL, the gradient is further from float64 than the fp64 form's; handles created without it are unchanged."""
    case = ("noise", "up", 3, 4100)
    est, ref = D.case(*case)
    l64, a64, _ = D.spec_reference(est, ref, D.STFT, torch.float64, key=case)
    v, ga, _ = _run(_module(D.STFT), est, ref, need_ref=False)
    monkeypatch.setenv("ESCX_SPEC_LOSS_F32", "1")
    v32, ga32, _ = _run(_module(D.STFT), est, ref, need_ref=False)            # a new module: a new handle
    monkeypatch.delenv("ESCX_SPEC_LOSS_F32")
    v2, ga2, _ = _run(_module(D.STFT), est, ref, need_ref=False)
    assert D.rel_err([v32], [float(l64)]) <= D.LOSS_RTOL
    assert not np.array_equal(ga32, ga) and D.rel_rms(ga32, a64) > D.rel_rms(ga, a64)
    assert v2 == v and np.array_equal(ga2, ga)


def test_c_abi_refuses_bad_arguments():
    from esc import _native
    lib = _native.load()
    E = _native.ESCX_ERR_INVALID_ARG
    cfg = _native.EscxSpecLossConfig()
    cfg.n_scales, cfg.clamp_eps, cfg.pow, cfg.mag_weight, cfg.log_weight = 1, 1e-5, 2.0, 1.0, 1.0
    cfg.window[0] = 64
    h = ctypes.c_void_p()
    for w in (0, -4, 30, 66):
        cfg.window[0] = w
        assert lib.escx_spec_loss_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == E and not h.value
    cfg.window[0], cfg.n_mels[0] = 64, 10
    assert lib.escx_spec_loss_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == E            # n_mels without a filterbank
    cfg.n_mels[0] = 0
    assert lib.escx_spec_loss_create(ctypes.byref(cfg), 0, None) == E
    assert lib.escx_spec_loss_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == 0 and h.value
    x = torch.randn(2, 100, device=DEV)
    out = torch.full((1,), 7.0, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert lib.escx_spec_loss_workspace_floats(h, 2, 100, 1, 1) > lib.escx_spec_loss_workspace_floats(h, 2, 100, 0, 0) > 0
    assert lib.escx_spec_loss_workspace_floats(h, 2, 32, 1, 1) == -1
    for args in ((None, p(x), p(x), 2, 100, p(out)), (h, None, p(x), 2, 100, p(out)), (h, p(x), None, 2, 100, p(out)), (h, p(x), p(x), 2, 100, None),
                 (h, p(x), p(x), 0, 100, p(out)), (h, p(x), p(x), 2, 32, p(out))):
        assert lib.escx_spec_loss_eval(*args, None, None, None) == E
    assert lib.escx_wave_l1(None, p(x), 200, 1.0, p(out), None, None, None) == E and lib.escx_wave_l1(p(x), p(x), 0, 1.0, p(out), None, None, None) == E
    assert lib.escx_sisdr(p(x), None, 2, 100, 1, 1, 0, 0.0, p(out), None, None, None) == E and lib.escx_sisdr(p(x), p(x), 0, 100, 1, 1, 0, 0.0, p(out), None, None, None) == E
    torch.cuda.synchronize()
    assert float(out) == 7.0                                                                # nothing was launched
    assert lib.escx_spec_loss_eval(h, p(x), p(x), 2, 100, p(out), None, None, None) == 0
    torch.cuda.synchronize()
    assert float(out) == 0.0
    lib.escx_spec_loss_destroy(h)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("n", D.L1_SIZES)
def test_l1_loss(B, n):
    from esc.baselines import L1Loss
    est, ref, ties = D.l1_case(B, n)
    for reduction in ("mean", "sum"):
        l64, a64, b64 = D.with_grads(lambda a, b: D.wave_l1(a, b, reduction), est, ref, torch.float64)
        v, ga, gb = _run(L1Loss(reduction=reduction), est, ref)
        assert D.rel_err([v], [float(l64)]) <= D.LOSS_RTOL
        scale = np.float32(1.0 / (B * n)) if reduction == "mean" else np.float32(1.0)
        assert np.array_equal(ga, np.sign(a64) * np.float64(scale)) and np.array_equal(gb, -ga)          # exact in sign and scale
        assert not ga[ties.numpy()].any() and ga[~ties.numpy()].all() if (~ties).any() else not ga.any()
    v, ga, gb = _run(L1Loss(), est, ref, need_ref=False)
    assert gb is None and ga is not None


@pytest.mark.parametrize("B,L", D.SISDR_SHAPES)
def test_sisdr_loss(B, L):
    from esc.baselines import SISDRLoss
    references, estimates = D.sisdr_case(B, L)
    clipped = 0
    for scaling, zero_mean, clip_min in D.SISDR_OPTIONS:
        per64 = D.sisdr(references.double(), estimates.double(), scaling, zero_mean, clip_min).numpy()
        clipped += int(clip_min is not None and (per64 == clip_min).any())
        for reduction in D.REDUCTIONS:
            w = D.sisdr_weights(B) if reduction == "none" else None
            fn = lambda r, e: D.reduce(D.sisdr(r, e, scaling, zero_mean, clip_min), reduction)
            l64, r64, e64 = D.with_grads(fn, references, estimates, torch.float64, w)
            loss = SISDRLoss(scaling=scaling, reduction=reduction, zero_mean=zero_mean, clip_min=clip_min)
            r = references.to(DEV).requires_grad_(True)
            e = estimates.to(DEV).requires_grad_(True)
            v = loss(r, e)
            assert v.shape == ((B,) if reduction == "none" else ())
            (v * torch.as_tensor(w, dtype=torch.float32, device=DEV)).sum().backward() if reduction == "none" else v.backward()
            tag = f"scaling={scaling} zero_mean={zero_mean} clip_min={clip_min} {reduction}"
            assert D.rel_err(v.detach().cpu().numpy().reshape(-1), np.asarray(l64).reshape(-1)) <= D.LOSS_RTOL, tag
            assert D.rel_rms(r.grad.cpu().numpy(), r64) <= D.GRAD_TOL and D.rel_rms(e.grad.cpu().numpy(), e64) <= D.GRAD_TOL, tag
            if clip_min is not None and B > 1:
                assert not r.grad[B - 1].any() and not e.grad[B - 1].any(), tag                          # below clip_min: no gradient
    assert clipped == (4 if B > 1 else 0)


def test_golden_cases_through_the_device():
    from esc.baselines import L1Loss, SISDRLoss
    g = np.load(os.path.join(GOLDEN, "dac_loss.npz"))
    est, ref, est_wave = torch.from_numpy(g["est"]), torch.from_numpy(g["ref"]), torch.from_numpy(g["est_wave"])
    for name in ("yml", "defaults", "two", "stft"):
        v, ga, gb = _run(_module(D.CONFIGS[name]), est, ref)
        assert D.rel_err([v], [float(g[f"{name}_loss"])]) <= D.LOSS_RTOL, name
        ta = tb = D.GRAD_TOL
        if name == "stft":              # the STFT loss's bound: max(GRAD_TOL, 2 x the float32 restatement's error on the same case), measured against the fixture
            _, a32, b32 = D.spec_reference(est, ref, D.STFT, torch.float32)
            ta, tb = max(ta, 2 * D.rel_rms(a32, g["stft_d_est"])), max(tb, 2 * D.rel_rms(b32, g["stft_d_ref"]))
        ea, eb = D.rel_rms(ga, g[f"{name}_d_est"]), D.rel_rms(gb, g[f"{name}_d_ref"])
        print(f"[dac-loss fixture {name}] d_est {ea:.2e} (bound {ta:.2e})  d_ref {eb:.2e} (bound {tb:.2e})")
        assert ea <= ta and eb <= tb, name
    v, ga, gb = _run(L1Loss(), est_wave, ref)
    assert D.rel_err([v], [float(g["l1_loss"])]) <= D.LOSS_RTOL and D.rel_rms(ga, g["l1_d_est"]) <= D.GRAD_TOL and D.rel_rms(gb, g["l1_d_ref"]) <= D.GRAD_TOL
    v, gr, ge = _run(SISDRLoss(), ref, est_wave)
    assert D.rel_err([v], [float(g["sisdr_loss"])]) <= D.LOSS_RTOL and D.rel_rms(gr, g["sisdr_d_ref"]) <= D.GRAD_TOL and D.rel_rms(ge, g["sisdr_d_est"]) <= D.GRAD_TOL


def _tiny_model():
    import json
    from esc import synth
    from esc.baselines import DAC
    cfg = json.loads(str(np.load(os.path.join(GOLDEN, "dac_tiny.npz"))["config_json"]))
    model = DAC(**cfg)
    man = json.load(open(os.path.join(GOLDEN, "dac_tiny_manifest.json")))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.dac_state_dict(man).items()}, strict=True)
    return model.to(DEV).eval()


def test_one_trainer_step_on_dac_tiny():
    """scripts/train_dac.py's step on synthetic DAC-Tiny, 2 clips x 2560 samples: the three waveform / spectral loss values against the float64 restatement applied to
    the native forward's audio, the two VQ losses against the float64 restatement of the codec, the total against the weighted sum of the five restated values, a finite gradient for every parameter, and d total / d audio = the lambda-weighted sum of the three unit gradients."""
    from scripts import train_dac as T
    model = _tiny_model()
    model.quantizer_dropout = 0.5                  # the yml's; the fixture's configuration leaves it off
    model.set_trainable("decoder").set_encode_trainable("both")
    losses = T.make_losses(T.YML_LOSSES, model.sample_rate)
    signal = full_signal = (0.1 * torch.randn(2, 1, 2560, generator=torch.Generator().manual_seed(3))).to(DEV)
    nq = model.sample_n_quantizers(2, torch.Generator().manual_seed(3))                 # [5, 18]: the first clip drops codebooks
    lam = dict(T.LAMBDAS, **{"stft/loss": 0.5, "waveform/loss": 2.0})           # the yml weighs only the mel loss: give the other two a weight as well
    hook = {}
    out = T.train_step_losses(model, losses, signal, nq, lam, audio_hook=lambda a: hook.setdefault("audio", a))
    out["loss"].backward()
    torch.cuda.synchronize()
    audio = hook["audio"]
    signal = signal[..., :audio.shape[-1]]                    # the trainer's cut: these decoder rates return 8 samples fewer than they take
    assert audio.shape == (2, 1, 2552)
    a64, s64 = audio.detach().cpu().double()[:, 0], signal.cpu().double()[:, 0]
    want = {"mel/loss": D.spectral_loss(a64, s64, D.YML), "stft/loss": D.spectral_loss(a64, s64, D.STFT), "waveform/loss": D.wave_l1(a64, s64)}
    for k, w in want.items():
        assert D.rel_err([float(out[k].detach())], [float(w)]) <= D.LOSS_RTOL, k
    # the two VQ losses: the float64 restatement of the codec (tests/dac_encode_grad_util.DacRefE: the reference quantiser with per-clip counts) on the same
    # weights, signal and n_quantizers, continued from the device's codes - a near-tie resolved the other way legitimately changes a loss, and which code is
    # chosen is tests/test_dac.py's subject
    with torch.no_grad():
        codes = model(full_signal, n_quantizers=nq)["codes"].cpu()
    ref = eu.DacRefE(eu.config("dac_tiny"), {k: v.detach().cpu() for k, v in model.state_dict().items()}, torch.float64)
    x64 = torch.nn.functional.pad(full_signal.cpu().double(), (0, -full_signal.shape[-1] % ref.hop))
    with torch.no_grad():
        enc = ref.encode_dict(x64, max(nq), codes, torch.tensor(nq))
    want.update({"vq/commitment_loss": enc["cm"], "vq/codebook_loss": enc["cb"]})
    assert float(enc["cm"]) > 0 and float(enc["cb"]) > 0 and min(nq) < max(nq) == model.n_codebooks
    for k in ("vq/commitment_loss", "vq/codebook_loss"):
        assert D.rel_err([float(out[k].detach())], [float(want[k])]) <= D.LOSS_RTOL, k
    total = sum(lam[k] * float(want[k]) for k in lam if k in want)             # the expected total from the RESTATED values
    assert set(want) == {k for k in lam if k in out} and len(want) == 5
    assert D.rel_err([float(out["loss"].detach())], [total]) <= D.LOSS_RTOL
    for key, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), key
    units = 0
    for k, loss in (("mel/loss", losses["mel"]), ("stft/loss", losses["stft"]), ("waveform/loss", losses["waveform"])):
        a = audio.detach().clone().requires_grad_(True)
        loss(a, signal).backward()
        units = units + lam[k] * a.grad
    assert D.rel_rms(audio.grad.cpu().numpy(), units.cpu().numpy()) <= 1e-6


def test_train_dac_script_writes_a_loadable_checkpoint(tmp_path):
    from esc.baselines import DAC
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "efficient-speech-codec_amd"))
    r = subprocess.run([sys.executable, "-m", "scripts.train_dac", "--synthetic", "dac_tiny", "--steps", "2", "--batch_size", "2", "--save_path", str(tmp_path)],
                       cwd=os.path.join(ROOT, "efficient-speech-codec_amd"), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    path = tmp_path / "latest" / "dac" / "weights.pth"
    assert path.exists(), r.stdout
    model = DAC.load(str(path))
    ck = torch.load(str(path), map_location="cpu", weights_only=False)
    sd = model.state_dict()
    assert set(sd) == set(ck["state_dict"])
    for k, v in ck["state_dict"].items():
        assert torch.equal(sd[k], v), k
    assert "step 2" in r.stdout


def test_train_dac_script_reads_wav_files(tmp_path):
    """--data (a directory of wav files at the model's rate, cut into random clips), --duration and --valid_freq."""
    from scipy.io import wavfile
    from esc import synth
    data = tmp_path / "wavs"
    data.mkdir()
    wavfile.write(str(data / "a.wav"), 16000, synth.noise_clip_int16("train-dac-a", 4000))
    wavfile.write(str(data / "b.wav"), 16000, synth.voiced_clip_int16("train-dac-b", 6000))
    wavfile.write(str(data / "short.wav"), 16000, synth.noise_clip_int16("train-dac-c", 100))          # shorter than a clip: left out
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "efficient-speech-codec_amd"))
    cmd = [sys.executable, "-m", "scripts.train_dac", "--synthetic", "dac_tiny", "--steps", "2", "--batch_size", "2", "--seed", "1", "--data", str(data), "--duration", "0.2",
           "--valid_freq", "1", "--save_path", str(tmp_path / "out")]
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "efficient-speech-codec_amd"), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("test/mel/loss") == 2 and "clips of 3200 samples from 2 wav files" in r.stdout and (tmp_path / "out" / "latest" / "dac" / "weights.pth").exists()
    wavfile.write(str(data / "rate.wav"), 8000, synth.noise_clip_int16("train-dac-d", 4000))
    r = subprocess.run(cmd, cwd=os.path.join(ROOT, "efficient-speech-codec_amd"), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "8000 Hz" in r.stderr
