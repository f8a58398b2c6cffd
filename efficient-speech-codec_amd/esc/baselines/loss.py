"""Training losses of the DAC baseline (`dac/nn/loss.py:11-368`) on the MI355X: L1Loss, SISDRLoss, MultiScaleSTFTLoss, MelSpectrogramLoss, and GANLoss
over esc.models.Discriminator (at the end of this file; escx_gan_term through esc.modules.loss._GanTermFn).

Same classes, constructor keywords, defaults and call order as the reference: `loss(x, y)` with x the estimate and y the reference signal (SISDRLoss
names its first argument `references`, as the reference does).  The arithmetic and the gradients run in libescx.so (include/escx.h escx_spec_loss_eval,
escx_wave_l1, escx_sisdr); each forward evaluates the unit gradients of whichever sides require one and backward only scales them, like esc.modules'
losses.  Arguments are float32 HIP tensors (B, 1, L) or (B, L), or any object with an `.audio_data` attribute holding one; the result is a 0-dim tensor.

The filterbanks are librosa's `filters.mel` with its defaults (Slaney scale, norm="slaney"), computed here in float64 and handed to the library as
float32 data; the two spectral classes take `sample_rate` as a constructor keyword (the reference reads it from the AudioSignal).
"""
from __future__ import annotations

import ctypes
import typing
from typing import List

import numpy as np
import torch
from torch import nn

from .. import _native
from ..models.discriminator import _buffer_plan
from ..modules.loss import _GanTermFn, _by_buffer

__all__ = ["L1Loss", "SISDRLoss", "MultiScaleSTFTLoss", "MelSpectrogramLoss", "GANLoss", "slaney_filterbank"]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _signal(x, attribute="audio_data"):
    """The (B, L) view of an argument (differentiable) - a tensor (B, 1, L) / (B, L) or an object holding one in `.audio_data`."""
    if not isinstance(x, torch.Tensor):
        if not hasattr(x, attribute):
            raise TypeError(f"expected a tensor or an object with .{attribute}, got {type(x).__name__}")
        x = getattr(x, attribute)
    if not x.is_cuda:
        raise RuntimeError("esc.baselines losses run on a HIP device only (no CPU implementation in this package)")
    if x.dtype != torch.float32:
        raise TypeError(f"expected a float32 tensor, got {x.dtype}")
    if x.dim() == 3 and x.shape[1] == 1:
        return x.reshape(x.shape[0], x.shape[2])
    if x.dim() == 2:
        return x
    raise ValueError(f"expected audio of shape (B, 1, L) or (B, L), got {tuple(x.shape)}")


def _pair(x, y, attribute="audio_data"):
    a, b = _signal(x, attribute), _signal(y, attribute)
    if a.shape != b.shape or a.device != b.device:
        raise RuntimeError(f"the two signals differ: {tuple(a.shape)} on {a.device} and {tuple(b.shape)} on {b.device}")
    return a, b


def _scale(unit: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """unit (rows, n) * g (rows,) on the device (escx_scale_rows)."""
    lib = _native.load()
    g = g.to(torch.float32).reshape(-1).contiguous()
    out = torch.empty_like(unit)
    rows = g.numel()
    with torch.cuda.device(unit.device):
        _native.check(lib.escx_scale_rows(_ptr(unit), _ptr(g), _ptr(out), rows, unit.numel() // rows, _stream(unit.device)))
    return out


# ---- L1 ---------------------------------------------------------------------------------------------------------------------------------
class _WaveL1Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, mean):
        lib = _native.load()
        xc, yc = x.detach().contiguous(), y.detach().contiguous()
        n = xc.numel()
        loss = torch.empty((), dtype=torch.float32, device=xc.device)
        gx = torch.empty_like(xc) if ctx.needs_input_grad[0] else None
        gy = torch.empty_like(yc) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(xc.device):
            _native.check(lib.escx_wave_l1(_ptr(xc), _ptr(yc), n, (1.0 / n) if mean else 1.0, _ptr(loss), _ptr(gx), _ptr(gy), _stream(xc.device)))
        ctx.gx, ctx.gy = gx, gy
        return loss

    @staticmethod
    def backward(ctx, g):
        return (_scale(ctx.gx, g) if ctx.gx is not None else None, _scale(ctx.gy, g) if ctx.gy is not None else None, None)


class L1Loss(nn.L1Loss):
    """L1 loss between two signals (loss.py:11-48).  `reduction` "mean" (default) and "sum"; the elementwise form is not implemented."""

    def __init__(self, attribute: str = "audio_data", weight: float = 1.0, **kwargs):
        self.attribute = attribute
        self.weight = weight
        super().__init__(**kwargs)
        if self.reduction not in ("mean", "sum"):
            raise NotImplementedError(f"reduction={self.reduction!r}: L1Loss implements 'mean' and 'sum'")

    def forward(self, x, y):
        a, b = _pair(x, y, self.attribute)
        return _WaveL1Fn.apply(a, b, self.reduction == "mean")


# ---- SI-SDR -----------------------------------------------------------------------------------------------------------------------------
class _SisdrFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, references, estimates, scaling, zero_mean, clip_min):
        lib = _native.load()
        rc, ec = references.detach().contiguous(), estimates.detach().contiguous()
        B, L = rc.shape
        loss = torch.empty(B, dtype=torch.float32, device=rc.device)
        gr = torch.empty_like(rc) if ctx.needs_input_grad[0] else None
        ge = torch.empty_like(ec) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(rc.device):
            _native.check(lib.escx_sisdr(_ptr(rc), _ptr(ec), B, L, int(bool(scaling)), int(bool(zero_mean)), int(clip_min is not None),
                                         float(clip_min) if clip_min is not None else 0.0, _ptr(loss), _ptr(gr), _ptr(ge), _stream(rc.device)))
        ctx.gr, ctx.ge = gr, ge
        return loss

    @staticmethod
    def backward(ctx, g):
        return (_scale(ctx.gr, g) if ctx.gr is not None else None, _scale(ctx.ge, g) if ctx.ge is not None else None, None, None, None)


class SISDRLoss(nn.Module):
    """Scale-invariant source-to-distortion ratio (loss.py:51-139).  forward(x, y): x are the REFERENCES, y the estimates, as in the reference."""

    def __init__(self, scaling: int = True, reduction: str = "mean", zero_mean: int = True, clip_min: int = None, weight: float = 1.0):
        self.scaling = scaling
        self.reduction = reduction
        self.zero_mean = zero_mean
        self.clip_min = clip_min
        self.weight = weight
        super().__init__()

    def forward(self, x, y):
        references, estimates = _pair(x, y)
        sdr = _SisdrFn.apply(references, estimates, self.scaling, self.zero_mean, self.clip_min)
        if self.reduction == "mean":
            sdr = sdr.mean()
        elif self.reduction == "sum":
            sdr = sdr.sum()
        return sdr


# ---- the spectral losses ----------------------------------------------------------------------------------------------------------------
def _hz_to_mel(f):
    f = np.asarray(f, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(f >= min_log_hz, min_log_mel + np.log(np.maximum(f, 1e-300) / min_log_hz) / logstep, f / f_sp)


def _mel_to_hz(m):
    m = np.asarray(m, dtype=np.float64)
    f_sp = 200.0 / 3
    min_log_hz = 1000.0
    min_log_mel = min_log_hz / f_sp
    logstep = np.log(6.4) / 27.0
    return np.where(m >= min_log_mel, min_log_hz * np.exp(logstep * (m - min_log_mel)), f_sp * m)


def slaney_filterbank(sample_rate: int, n_fft: int, n_mels: int, fmin: float = 0.0, fmax: float = None) -> np.ndarray:
    """librosa.filters.mel(sr, n_fft, n_mels, fmin, fmax) with its defaults (htk=False, norm="slaney"): (n_mels, n_fft // 2 + 1) float32, computed in float64."""
    fmax = sample_rate / 2.0 if fmax is None else float(fmax)
    fftfreqs = np.fft.rfftfreq(n_fft, 1.0 / sample_rate)
    mel_f = _mel_to_hz(np.linspace(_hz_to_mel(float(fmin)), _hz_to_mel(fmax), n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = mel_f[:, None] - fftfreqs[None, :]
    lower = -ramps[:-2] / fdiff[:-1, None]
    upper = ramps[2:] / fdiff[1:, None]
    weights = np.maximum(0.0, np.minimum(lower, upper))
    weights *= (2.0 / (mel_f[2:n_mels + 2] - mel_f[:n_mels]))[:, None]
    return np.ascontiguousarray(weights.astype(np.float32))


class _Handle:
    """One escx_spec_loss on one device."""

    def __init__(self, device_index, windows, n_mels, banks, clamp_eps, pow, mag_weight, log_weight):
        lib = _native.load()
        cfg = _native.EscxSpecLossConfig()
        cfg.n_scales = len(windows)
        for i, (w, m, fb) in enumerate(zip(windows, n_mels, banks)):
            cfg.window[i], cfg.n_mels[i] = int(w), int(m)
            cfg.filterbank[i] = fb.ctypes.data if fb is not None else None
        cfg.clamp_eps, cfg.pow, cfg.mag_weight, cfg.log_weight = float(clamp_eps), float(pow), float(mag_weight), float(log_weight)
        h = ctypes.c_void_p()
        _native.check(lib.escx_spec_loss_create(ctypes.byref(cfg), int(device_index), ctypes.byref(h)))
        self.h, self._lib = h, lib

    def __del__(self):
        if getattr(self, "h", None):
            self._lib.escx_spec_loss_destroy(self.h)
            self.h = None


class _SpecLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, owner):
        lib = _native.load()
        xc, yc = x.detach().contiguous(), y.detach().contiguous()
        B, L = xc.shape
        if L <= owner.max_window // 2:
            raise ValueError(f"clips of {L} samples are too short for the {owner.max_window}-sample window (reflect padding needs more than half a window)")
        handle = owner._handle(xc.device)
        loss = torch.empty((), dtype=torch.float32, device=xc.device)
        gx = torch.empty_like(xc) if ctx.needs_input_grad[0] else None
        gy = torch.empty_like(yc) if ctx.needs_input_grad[1] else None
        with torch.cuda.device(xc.device):
            _native.check(lib.escx_spec_loss_eval(handle.h, _ptr(xc), _ptr(yc), B, L, _ptr(loss), _ptr(gx), _ptr(gy), _stream(xc.device)))
        ctx.gx, ctx.gy = gx, gy
        return loss

    @staticmethod
    def backward(ctx, g):
        return (_scale(ctx.gx, g) if ctx.gx is not None else None, _scale(ctx.gy, g) if ctx.gy is not None else None, None)


def _check_supported(loss_fn, match_stride, window_type):
    if type(loss_fn) is not nn.L1Loss or loss_fn.reduction != "mean":
        raise NotImplementedError(f"loss_fn={loss_fn!r}: only nn.L1Loss() is implemented")
    if match_stride:
        raise NotImplementedError("match_stride=True is not implemented")
    if window_type not in (None, "hann"):
        raise NotImplementedError(f"window_type={window_type!r}: only None / 'hann' is implemented")


class _SpectralLoss(nn.Module):
    def _scales(self):
        """[(window, n_mels, fmin, fmax)] of the scales the loss sums over; n_mels = 0: no filterbank."""
        raise NotImplementedError

    def __getstate__(self):                   # the native handles are per process: a copied or pickled loss makes its own
        state = self.__dict__.copy()
        state.pop("_handles", None)
        return state

    @property
    def max_window(self):
        return max(w for w, _, _, _ in self._scales())

    def _handle(self, device):
        idx = device.index if device.index is not None else torch.cuda.current_device()
        key = (idx, tuple((w, m, fmin, fmax) for w, m, fmin, fmax in self._scales()), float(self.clamp_eps), float(self.pow), float(self.mag_weight),
               float(self.log_weight), int(self.sample_rate))
        cache = self.__dict__.setdefault("_handles", {})
        if key not in cache:
            scales = self._scales()
            banks = [slaney_filterbank(self.sample_rate, w, m, fmin, fmax) if m else None for w, m, fmin, fmax in scales]
            for stale in [k for k in cache if k[0] == idx]:          # the attributes changed: this device's old handle is dropped
                del cache[stale]
            cache[key] =_Handle(idx, [s[0] for s in scales], [s[1] for s in scales], banks, self.clamp_eps, self.pow, self.mag_weight, self.log_weight)
        return cache[key]

    def forward(self, x, y):
        a, b = _pair(x, y)
        if not self._scales():
            return torch.zeros((), dtype=torch.float32, device=a.device)
        return _SpecLossFn.apply(a, b, self)


class MultiScaleSTFTLoss(_SpectralLoss):
    """Multi-scale STFT loss (loss.py:142-228): per window, log_weight * L1 of log10(clamp(|S|)^pow) + mag_weight * L1 of |S|."""

    def __init__(self, window_lengths: List[int] = [2048, 512], loss_fn: typing.Callable = nn.L1Loss(), clamp_eps: float = 1e-5, mag_weight: float = 1.0,
                 log_weight: float = 1.0, pow: float = 2.0, weight: float = 1.0, match_stride: bool = False, window_type: str = None,
                 sample_rate: int = 16000):
        super().__init__()
        _check_supported(loss_fn, match_stride, window_type)
        self.window_lengths = list(window_lengths)
        self.loss_fn = loss_fn
        self.log_weight = log_weight
        self.mag_weight = mag_weight
        self.clamp_eps = clamp_eps
        self.weight = weight
        self.pow = pow
        self.match_stride, self.window_type, self.sample_rate = match_stride, window_type, sample_rate

    def _scales(self):
        return [(int(w), 0, 0.0, None) for w in self.window_lengths]


class MelSpectrogramLoss(_SpectralLoss):
    """Multi-scale mel loss (loss.py:231-327).  The zip over n_mels / mel_fmin / mel_fmax / window_lengths stops at the shortest list, as in the reference
    (the defaults of mel_fmin / mel_fmax have two entries)."""

    def __init__(self, n_mels: List[int] = [150, 80], window_lengths: List[int] = [2048, 512], loss_fn: typing.Callable = nn.L1Loss(), clamp_eps: float = 1e-5,
                 mag_weight: float = 1.0, log_weight: float = 1.0, pow: float = 2.0, weight: float = 1.0, match_stride: bool = False,
                 mel_fmin: List[float] = [0.0, 0.0], mel_fmax: List[float] = [None, None], window_type: str = None, sample_rate: int = 16000):
        super().__init__()
        _check_supported(loss_fn, match_stride, window_type)
        self.window_lengths = list(window_lengths)
        self.n_mels = n_mels
        self.loss_fn = loss_fn
        self.clamp_eps = clamp_eps
        self.log_weight = log_weight
        self.mag_weight = mag_weight
        self.weight = weight
        self.mel_fmin = mel_fmin
        self.mel_fmax = mel_fmax
        self.pow = pow
        self.match_stride, self.window_type, self.sample_rate = match_stride, window_type, sample_rate

    def _scales(self):
        return [(int(w), int(m), float(fmin), None if fmax is None else float(fmax))
                for m, fmin, fmax, w in zip(self.n_mels, self.mel_fmin, self.mel_fmax, self.window_lengths)]


# ---- GAN ----------------------------------------------------------------------------------------------------------------------------------
class _DiscLossFn(torch.autograd.Function):
    """mean_b(sum over sub-discriminators of mean (0 - D(fake_b))^2 + mean (1 - D(real_b))^2) from ONE discriminator forward over [fake | real], differentiable
    in the discriminator's parameters.  The backward runs per half of that pass - clips [0, B), then [B, 2B): every buffer is batch-major, so a clip range of
    the pass is a pass - and adds the two parameter gradients.  That is the arithmetic of esc.modules.GANLoss.discriminator_loss, whose two halves are two
    passes: each half's weight gradients are reduced and rounded on their own.  One backward over all 2B clips sums the four clips before rounding and lands a
    few float32 ulps elsewhere on the norm gradients where the halves nearly cancel (1.3e-6 on one of 324 tensors of the yml's discriminator)."""

    @staticmethod
    def forward(ctx, disc, f, r, *params):
        B = f.shape[0]
        both = disc(torch.cat([f, r], dim=0).unsqueeze(1))
        loss = 0
        for sub in both:                        # the clip-range form: the pass's own buffer, clips [0, B) against 0 and [B, 2B) against 1
            buf, *meta = sub.entries[-1]
            loss = loss + _GanTermFn.apply(buf, None, (tuple(meta),), 0, 0.0, 0, B) + _GanTermFn.apply(buf, None, (tuple(meta),), 0, 1.0, B, B)
        ctx.disc, ctx.both, ctx.B = disc, both, B
        return loss.mean()

    @staticmethod
    def backward(ctx, g):
        disc, both, B = ctx.disc, ctx.both, ctx.B
        dev = both.wave.device
        lib, hd = disc._handle(dev)
        flat = disc._ensure_flat(dev, lib, hd)
        st = disc._flat[dev.index if dev.index is not None else torch.cuda.current_device()]
        scale = (g.to(torch.float32) / B).expand(B).contiguous()                 # d mean_b(term_b)
        total = None
        for lo, target in ((0, 0.0), (B, 1.0)):
            half = both.clips(lo, lo + B)
            dbufs = [None] * len(half.bufs)
            for sub in half:
                buf, C, Cp, D0, D1, P1, off1 = sub.entries[-1]             # the last map of a sub-discriminator is a buffer of its own
                grad = torch.empty_like(buf)
                with torch.cuda.device(dev):
                    _native.check(lib.escx_gan_term_grad(_ptr(buf), None, _ptr(scale), _ptr(grad), B, C, Cp, D0, D1, P1, 0, float(target), _stream(dev)))
                dbufs[next(i for i, b in enumerate(half.bufs) if b.data_ptr() == buf.data_ptr())] = grad
            gflat = torch.empty_like(flat)
            n = len(half.layout)
            _, where = _buffer_plan(half.layout)
            at = lambda bufs: (ctypes.c_void_p * n)(*[(None if bufs[bi] is None else bufs[bi].data_ptr() + 4 * off1 * half.layout[i][2])     # noqa: E731
                                                      for i, (bi, off1) in enumerate(where)])
            with torch.cuda.device(dev):
                _native.check(lib.escx_disc_backward(hd, _ptr(flat), disc._version(), _ptr(half.wave), B, half.wave.shape[1], at(half.bufs), at(dbufs), _ptr(gflat), None,
                                                     _stream(dev)))
            total = gflat if total is None else total + gflat
        if disc._flat_grad_mode and "gflat" in st:              # esc.optim.FlatAdamW: the parameters' .grad are views of one buffer, written in place
            st["gflat"].copy_(total) if st["gfresh"] else st["gflat"].add_(total)
            st["gfresh"] = False
            return (None,) * (3 + len(st["layout"]))
        params = dict(disc.named_parameters())
        by_id = {id(params[k]): total[off:off + n_].view(params[k].shape) for k, off, n_ in st["layout"]}
        return (None, None, None) + tuple(by_id.get(id(p)) for p in disc.parameters())


class GANLoss(nn.Module):
    """Least-squares GAN and feature-matching losses of the adversarial recipe (loss.py:330-368) over esc.models.Discriminator, the reference's
    `dac.model.Discriminator`.  `discriminator_loss(fake, real)` -> 0-dim; `generator_loss(fake, real)` -> (loss_g, loss_feature), both 0-dim.

    The reference takes `torch.mean` over whole maps; the terms here are evaluated per clip on the discriminator's channels-last buffers (escx_gan_term, no
    NCHW map is materialised) and averaged over the batch, which is the same number for clips of one length.  Each loss call runs the discriminator ONCE,
    over [fake | real]: a clip's maps do not depend on the batch it is in, so the values are those of the reference's two passes (the discriminator's
    parameter gradients too: _DiscLossFn runs the backward of that one forward per half).  Signals of unequal shape take
    two passes in `discriminator_loss`; `generator_loss` refuses them (the feature-matching term compares maps of equal size, in the reference as well).

    What is differentiable: `discriminator_loss` in the discriminator's parameters only (fake is detached as in the reference, and real is data);
    `generator_loss` in `fake` only.  One departure from the reference: its `generator_loss(...)` backward also deposits gradients in the discriminator's
    parameters, which its trainer then discards (`optimizer_d.zero_grad()` precedes every discriminator backward, train_customize.py:286); here the
    discriminator's `p.grad` are left untouched by `generator_loss` and its backward."""

    def __init__(self, discriminator):
        super().__init__()
        self.discriminator = discriminator

    def forward(self, fake, real):
        """(d_fake, d_real): the discriminator's feature maps of both signals, as the reference returns them (two passes, fully differentiable)."""
        return self.discriminator(_signal(fake).unsqueeze(1)), self.discriminator(_signal(real).unsqueeze(1))

    def discriminator_loss(self, fake, real):
        f, r = _signal(fake).detach(), _signal(real).detach()
        if f.shape != r.shape:
            d_fake, d_real = self.discriminator(f.unsqueeze(1)), self.discriminator(r.unsqueeze(1))
            loss = 0
            for xf, xr in zip(d_fake, d_real):
                (bf, *mf), (br, *mr) = xf.entries[-1], xr.entries[-1]
                loss = loss + _GanTermFn.apply(bf, None, (tuple(mf),), 0, 0.0).mean() + _GanTermFn.apply(br, None, (tuple(mr),), 0, 1.0).mean()
            return loss
        return _DiscLossFn.apply(self.discriminator, f, r, *self.discriminator.parameters())

    def generator_loss(self, fake, real):
        f, r = _pair(fake, real)
        B = f.shape[0]
        both = self.discriminator(torch.cat([f, r.detach()], dim=0).unsqueeze(1), detach_params=True, grad_clips=B)
        loss_g, loss_f = 0, 0
        for sub in both:
            buf, *meta = sub.entries[-1]
            loss_g = loss_g + _GanTermFn.apply(buf, None, (tuple(meta),), 0, 1.0, 0, B)
            for buf, metas in _by_buffer(sub.entries[:-1]):
                loss_f = loss_f + _GanTermFn.apply(buf, buf.detach()[B:], tuple(metas), 1, 0.0, 0, B)
        return loss_g.mean(), loss_f.mean()
