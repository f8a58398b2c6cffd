"""Inputs and references of the DAC-loss tests (test_dac_loss_host.py on the host, test_dac_loss.py on the GPU).

Everything here runs on the CPU.  The references are a torch restatement of the four losses of the DAC baseline (`dac/nn/loss.py:11-327`), evaluated in
float64 (the truth the kernels are held to) and in float32 (what the reference itself would give: the yardstick of the STFT-loss gradient bound and the
condition test_dac_loss_host.py checks for every other case).  The loss arithmetic (clamp, pow, log10, weights, zip truncation, batch mean, L1, SI-SDR) is
pinned to the real reference by tests/golden/dac_loss.npz (tools/gen_dac_loss_golden.py); the STFT (torch.stft, periodic hann, center=True, reflect padding -
audiotools' convention) and the Slaney filterbank (librosa.filters.mel with its defaults) are restated here, not pinned: neither package is installed where
the fixture was written.

The gradient cases use scaled reconstructions (rec = gain x raw), for the reason loss_util.py gives: an L1 of (log-)magnitudes has a gradient of signs, and
independent noise produces near-ties.  margins() measures the distance from a tie and the host test asserts it.
"""
import math

import numpy as np
import torch

import loss_util as U

LOSS_RTOL, GRAD_TOL, TIE_MARGIN = U.LOSS_RTOL, U.GRAD_TOL, U.TIE_MARGIN
SR = 16000

# ---- configurations -----------------------------------------------------------------------------------
YML = dict(name="yml", n_mels=[5, 10, 20, 40, 80, 160, 320], window_lengths=[32, 64, 128, 256, 512, 1024, 2048], mel_fmin=[0, 0, 0, 0, 0, 0, 0],
           mel_fmax=[None] * 7, pow=1.0, clamp_eps=1e-5, mag_weight=0.0, log_weight=1.0)                     # conf/16khz_dns_9k.yml
DEFAULTS = dict(name="defaults", n_mels=[150, 80], window_lengths=[2048, 512], mel_fmin=[0.0, 0.0], mel_fmax=[None, None], pow=2.0, clamp_eps=1e-5,
                mag_weight=1.0, log_weight=1.0)                                                              # loss.py:259-273
TWO = dict(name="two", n_mels=[10, 40], window_lengths=[64, 256], mel_fmin=[0.0, 0.0], mel_fmax=[None, None], pow=1.0, clamp_eps=1e-5, mag_weight=0.5,
           log_weight=2.0)
STFT = dict(name="stft", n_mels=None, window_lengths=[2048, 512], pow=2.0, clamp_eps=1e-5, mag_weight=1.0, log_weight=1.0)      # loss.py:174-185
MEL_CONFIGS = (YML, DEFAULTS, TWO)
CONFIGS = {c["name"]: c for c in (YML, DEFAULTS, TWO, STFT)}


def with_(cfg, **kw):
    out = dict(cfg)
    out.update(kw)
    return out


def scales(cfg):
    """[(window, n_mels or 0, fmin, fmax)]: the zip of the reference stops at the shortest list."""
    if cfg["n_mels"] is None:
        return [(w, 0, 0.0, None) for w in cfg["window_lengths"]]
    return [(w, m, fmin, fmax) for m, fmin, fmax, w in zip(cfg["n_mels"], cfg["mel_fmin"], cfg["mel_fmax"], cfg["window_lengths"])]


def module_kwargs(cfg):
    return {k: v for k, v in cfg.items() if k != "name" and not (k == "n_mels" and v is None)}


# ---- the Slaney filterbank (librosa.filters.mel, htk=False, norm="slaney") ----------------------------
def _hz_to_mel(f):
    f = np.asarray(f, np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), f * 3.0 / 200.0)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), m * 200.0 / 3.0)


_FB = {}


def slaney(n_fft, n_mels, fmin=0.0, fmax=None, sr=SR):
    """(n_mels, n_fft // 2 + 1) float32, computed in float64."""
    key = (n_fft, n_mels, fmin, fmax, sr)
    if key not in _FB:
        fmax_ = sr / 2.0 if fmax is None else float(fmax)
        freqs = np.arange(n_fft // 2 + 1, dtype=np.float64) * sr / n_fft
        pts = _mel_to_hz(np.linspace(float(_hz_to_mel(float(fmin))), float(_hz_to_mel(fmax_)), n_mels + 2))
        fb = np.zeros((n_mels, freqs.size))
        for i in range(n_mels):
            lower = (freqs - pts[i]) / (pts[i + 1] - pts[i])
            upper = (pts[i + 2] - freqs) / (pts[i + 2] - pts[i + 1])
            fb[i] = np.maximum(0.0, np.minimum(lower, upper)) * 2.0 / (pts[i + 2] - pts[i])
        _FB[key] = fb.astype(np.float32)
    return _FB[key]


# ---- the restatement ----------------------------------------------------------------------------------
_CONST = {}


def _tensor(key, like, make):
    """A constant (window, filterbank) in `like`'s dtype on its device, made once."""
    k = (key, like.dtype, str(like.device))
    if k not in _CONST:
        _CONST[k] = make().to(like.device)
    return _CONST[k]


def magnitude(x, w):
    """|STFT| (B, F, T) of x (B, L) in x's dtype: hop w / 4, periodic hann, center=True, reflect padding."""
    win = _tensor(("hann", w), x, lambda: torch.hann_window(w, periodic=True, dtype=x.dtype))
    return torch.stft(x, n_fft=w, hop_length=w // 4, win_length=w, window=win, center=True, pad_mode="reflect", return_complex=True).abs()


def features(x, w, n_mels, fmin=0.0, fmax=None, sr=SR):
    """(B, T, bins): the magnitude (n_mels = 0) or the mel spectrogram, as audiotools lays them out after its transpose."""
    m = magnitude(x, w).transpose(1, 2)
    if n_mels:
        m = m @ _tensor(("fb", w, n_mels, fmin, fmax, sr), x, lambda: torch.from_numpy(slaney(w, n_mels, fmin, fmax, sr)).to(x.dtype)).T
    return m


def spectral_loss(x, y, cfg, sr=SR):
    """MelSpectrogramLoss / MultiScaleSTFTLoss of the estimate x against the reference y, (B, L) each; 0-dim."""
    l1 = torch.nn.functional.l1_loss
    loss = 0.0
    for w, nm, fmin, fmax in scales(cfg):
        xm, ym = features(x, w, nm, fmin, fmax, sr), features(y, w, nm, fmin, fmax, sr)
        loss = loss + cfg["log_weight"] * l1(xm.clamp(cfg["clamp_eps"]).pow(cfg["pow"]).log10(), ym.clamp(cfg["clamp_eps"]).pow(cfg["pow"]).log10())
        loss = loss + cfg["mag_weight"] * l1(xm, ym)
    return loss


def wave_l1(x, y, reduction="mean"):
    return torch.nn.functional.l1_loss(x, y, reduction=reduction)


def sisdr(references, estimates, scaling=True, zero_mean=True, clip_min=None):
    """loss.py:91-133 up to the reduction: (B,)."""
    eps = 1e-8
    nb = references.shape[0]
    references = references.reshape(nb, 1, -1).permute(0, 2, 1)
    estimates = estimates.reshape(nb, 1, -1).permute(0, 2, 1)
    mr = references.mean(dim=1, keepdim=True) if zero_mean else 0
    me = estimates.mean(dim=1, keepdim=True) if zero_mean else 0
    r, e = references - mr, estimates - me
    proj = (r ** 2).sum(dim=-2) + eps
    on = (e * r).sum(dim=-2) + eps
    scale = (on / proj).unsqueeze(1) if scaling else 1
    e_true = scale * r
    e_res = e - e_true
    sdr = -10 * torch.log10((e_true ** 2).sum(dim=1) / (e_res ** 2).sum(dim=1) + eps)
    if clip_min is not None:
        sdr = torch.clamp(sdr, min=clip_min)
    return sdr.reshape(nb)


def reduce(v, reduction):
    return v.mean() if reduction == "mean" else (v.sum() if reduction == "sum" else v)


def with_grads(fn, a, b, dtype, weights=None):
    """(value, d / d a, d / d b) as float64 arrays of fn(a, b) evaluated in `dtype`; a vector value is contracted with `weights` (default ones)."""
    a = a.detach().to(dtype).requires_grad_(True)
    b = b.detach().to(dtype).requires_grad_(True)
    v = fn(a, b)
    w = torch.ones_like(v) if weights is None else torch.as_tensor(weights).to(dtype)
    (v * w).sum().backward()
    z = lambda t: np.zeros(tuple(t.shape)) if t.grad is None else t.grad.double().numpy()
    return v.detach().double().numpy(), z(a), z(b)


_REF = {}


def spec_reference(est, ref, cfg, dtype=torch.float64, key=None):
    """(loss, d_est, d_ref) float64 arrays; cached under `key` (computed once, shared by the tests, never modified)."""
    k = None if key is None else (key, cfg["name"], dtype)
    if k is not None and k in _REF:
        return _REF[k]
    out = with_grads(lambda a, b: spectral_loss(a, b, cfg), est, ref, dtype)
    if k is not None:
        _REF[k] = out
    return out


# ---- margins ------------------------------------------------------------------------------------------
def margins(est, ref, cfg):
    """Distance of a spectral-loss input from the points where its gradient jumps, in float64 over the configuration's scales:
    (min |x - y| / (x + y) where the linear term is on,  min |lx - ly| over cells with a side above the clamp where the log term is on,
     min |v - clamp| / clamp over both sides where the log term is on).  Cells where both sides are exactly 0 carry no gradient (first measure)."""
    lin, log, clamp = math.inf, math.inf, math.inf
    est, ref = est.double(), ref.double()
    eps, p = cfg["clamp_eps"], cfg["pow"]
    for w, nm, fmin, fmax in scales(cfg):
        x, y = features(est, w, nm, fmin, fmax), features(ref, w, nm, fmin, fmax)
        if cfg["mag_weight"] != 0:
            live = (x + y) > 0
            if live.any():
                lin = min(lin, float(((x - y).abs()[live] / (x + y)[live]).min()))
        if cfg["log_weight"] != 0:
            above = (x >= eps) | (y >= eps)
            if above.any():
                lx, ly = x.clamp(eps).pow(p).log10(), y.clamp(eps).pow(p).log10()
                log = min(log, float((lx - ly).abs()[above].min()))
            for v in (x, y):
                clamp = min(clamp, float(((v - eps).abs() / eps).min()))
    return lin, log, clamp


def clamp_straddles(est, ref, cfg):
    """(cells with est < clamp <= ref, cells with ref < clamp <= est) over the scales, float64."""
    n_e, n_r = 0, 0
    est, ref = est.double(), ref.double()
    eps = cfg["clamp_eps"]
    for w, nm, fmin, fmax in scales(cfg):
        x, y = features(est, w, nm, fmin, fmax), features(ref, w, nm, fmin, fmax)
        n_e += int(((x < eps) & (y >= eps)).sum())
        n_r += int(((y < eps) & (x >= eps)).sum())
    return n_e, n_r


# ---- cases --------------------------------------------------------------------------------------------
SHAPES = ((1, 1025), (3, 1026), (2, 2049), (3, 4100))        # L = largest window / 2 + 1; L no multiple of any hop; B = 1


# (configuration, kind, gain, B, L) -> seed of a clip drawn again: with loss_util.mel_case's own seed the yml case below has one mel cell 1.5e-5 above the clamp
# on the estimate's side and clamped on the other - with pow = 1 a log difference of 6.4e-6, under TIE_MARGIN.  Seed 7002: log margin 5.2e-4, clamp margin 1.9e-4.
RESEED = {("yml", "quiet", "up", 2, 2049): 7002}


def case(kind, gain, B, L, name=None):
    """(est, ref) float32 (B, L): loss_util.mel_case's (raw, gain x raw) with the ESTIMATE first; `name`: the configuration the case is for (RESEED)."""
    raw, rec = U.mel_case(kind, gain, B, L, RESEED.get((name, kind, gain, B, L)))
    return rec, raw


# The well-conditioned cases of the filterbank configurations: noise and quiet clips x gains half / up / step at the four shapes, without
# (quiet, half, 1, 1025) for yml and defaults (a mel cell 1.8e-6 from the clamp).
def mel_cases(cfg):
    out = [(k, g, B, L) for k in ("noise", "quiet") for g in U.GAINS for B, L in SHAPES]
    if cfg["name"] in ("yml", "defaults"):
        out.remove(("quiet", "half", 1, 1025))
    return out


# The STFT loss: constant gains only (a step gain leaves cells 5e-6 from a linear tie).
STFT_CASES = [(k, g, B, L) for k in ("noise", "quiet") for g in ("half", "up") for B, L in SHAPES]
AT_CLAMP = ("at_clamp", 2, 2049)
AT_CLAMP_MIN_CELLS = U.MEL_AT_CLAMP_MIN_CELLS

L1_SIZES = (1, 255, 256, 257, 16385)


def l1_case(B, n, seed=None):
    """(est, ref, ties) float32 (B, n): noise with planted exact ties (est == ref) at the head, the middle and the tail of every clip."""
    g = torch.Generator().manual_seed(4000 + 3 * n + B if seed is None else seed)
    ref = torch.randn(B, n, generator=g)
    est = ref + 0.3 * torch.randn(B, n, generator=g)
    ties = torch.zeros(B, n, dtype=torch.bool)
    for b in range(B):
        for pos in {0, n // 2, n - 1, (7 + b) % n}:
            ties[b, pos] = True
    est = torch.where(ties, ref, est)
    return est, ref, ties


SISDR_SHAPES = ((1, 257), (3, 4100))
SISDR_OPTIONS = [(s, z, c) for s in (True, False) for z in (True, False) for c in (None, -30.0)]
REDUCTIONS = ("mean", "sum", "none")


def sisdr_case(B, L, seed=None):
    """(references, estimates) float32 (B, L): estimates = references + 0.1 x noise (about -20 dB), with a small offset so that zero_mean matters; the last
    clip of a batch of several has a tenth of that noise (about -40 dB: below clip_min = -30)."""
    g = torch.Generator().manual_seed(5000 + L + B if seed is None else seed)
    references = 0.1 * torch.randn(B, L, generator=g) + 0.01
    noise = 0.01 * torch.randn(B, L, generator=g)
    if B > 1:
        noise[B - 1] *= 0.1
    estimates = references + noise - 0.0003
    return references, estimates


def sisdr_weights(B):
    return np.linspace(0.5, 1.5, B) if B > 1 else np.ones(1)


rel_rms, rel_err = U.rel_rms, U.rel_err
