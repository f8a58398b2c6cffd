"""Evaluation metrics of the reference (`/root/reference/scripts/metrics.py:12-171`) on the MI355X, with per-clip lengths.

  MelSpectrogramDistance  metrics.py:96-121   forward(x, y, lengths=None) -> (B,)   escx_mel_distance
  SISDR                   metrics.py:123-171  forward(x, y, lengths=None) -> (B,)   escx_sisdr_metric
  EntropyCounter          metrics.py:12-77    update(codes) skips the -1 filler      escx_code_histogram

Without `lengths` the two modules are drop-in for the classes of `scripts.metrics` (which stay the plain-torch yardstick).  With `lengths`
(a length-B sequence or 1-D integer tensor of sample counts) the batch is a zero-padded one: clip b is x[b, :lengths[b]], what is stored
past it is not read in either signal, and the clip gets the value of the call on the clip alone - its own reflect point and frame count in
the STFTs, its own divisors in the means.  The arithmetic runs in libescx.so; there is no CPU implementation.
"""
from __future__ import annotations

import ctypes
import math

import torch
import torch.nn as nn

from . import _native
from .models.codecs import ESC

MEL_WINDOWS = [32, 64, 128, 256, 512, 1024, 2048]
MEL_BINS = [5, 10, 20, 40, 80, 160, 320]
SR = 16000
MEL_MIN_SAMPLES = 1024          # half the longest window: torch.stft(center=True) reflects that many samples, so a clip is longer


def _need_gpu(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"esc.metrics (MI355X build): {what} must live on a HIP device (got {t.device}); this package has no CPU implementation of the metrics")


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _pair(x, y, what):
    """(B, L) views of the two signals; anything that is not two equal-shaped batches is a ValueError."""
    if not isinstance(x, torch.Tensor) or not isinstance(y, torch.Tensor):
        raise ValueError(f"{what} takes two tensors")
    if x.dim() < 2 or x.shape != y.shape:
        raise ValueError(f"{what}: x {tuple(x.shape)} and y {tuple(y.shape)} must both be (B, L)")
    return x.reshape(x.shape[0], -1), y.reshape(y.shape[0], -1)


def _lengths(lengths, B, lo, L):
    """None, or B integers in (lo, L] as a ctypes array; the message of a length outside the range names the clip."""
    if lengths is None:
        return None
    vals = ESC._int_list(lengths, "lengths", B)
    for b, v in enumerate(vals):
        if not lo < v <= L:
            raise ValueError(f"lengths[{b}]={v} outside ({lo}, {L}]")
    return (ctypes.c_int32 * B)(*vals)


class MelSpectrogramDistance(nn.Module):
    """L1 log-mel distance summed over 7 resolutions (metrics.py:96-121).  (B, L) x (B, L) -> (B,) float32 on the device."""

    def __init__(self, win_lengths=MEL_WINDOWS, n_mels=MEL_BINS, clamp_eps=1e-5, sample_rate=SR):
        super().__init__()
        if list(win_lengths) != MEL_WINDOWS or list(n_mels) != MEL_BINS or clamp_eps != 1e-5:
            raise NotImplementedError("the HIP mel distance implements the reference's fixed resolutions (metrics.py:100-104)")
        self.clamp_eps, self.sample_rate = clamp_eps, int(sample_rate)

    def forward(self, raw_audio, recon_audio, lengths=None):
        x, y = _pair(raw_audio, recon_audio, "MelSpectrogramDistance")
        if raw_audio.dim() != 2:
            raise ValueError(f"MelSpectrogramDistance: x {tuple(raw_audio.shape)} must be (B, L)")
        B, L = x.shape
        if L <= MEL_MIN_SAMPLES:
            raise ValueError(f"MelSpectrogramDistance: {L} samples are too short for the 2048-sample window (more than {MEL_MIN_SAMPLES} needed)")
        lens = _lengths(lengths, B, MEL_MIN_SAMPLES, L)
        _need_gpu(x, "x"); _need_gpu(y, "y")
        x, y = x.detach().to(torch.float32).contiguous(), y.detach().to(device=x.device, dtype=torch.float32).contiguous()
        out = torch.empty(B, dtype=torch.float32, device=x.device)
        if B == 0:
            return out
        lib = _native.load()
        with torch.cuda.device(x.device):
            _native.check(lib.escx_mel_distance(x.data_ptr(), y.data_ptr(), B, L, lens, self.sample_rate, out.data_ptr(), _stream(x.device)))
        return out


class SISDR(nn.Module):
    """Scale-invariant source-to-distortion ratio in dB, (B, L) x (B, L) -> (B,) float32 on the device (metrics.py:123-171)."""

    def __init__(self, scaling: bool = True, zero_mean: bool = True):
        super().__init__()
        self.scaling, self.zero_mean = scaling, zero_mean

    def forward(self, x, y, lengths=None):
        ref, est = _pair(x, y, "SISDR")
        B, L = ref.shape
        if L < 1:
            raise ValueError("SISDR: empty clips")
        lens = _lengths(lengths, B, 0, L)
        _need_gpu(ref, "x"); _need_gpu(est, "y")
        ref, est = ref.detach().to(torch.float32).contiguous(), est.detach().to(device=ref.device, dtype=torch.float32).contiguous()
        out = torch.empty(B, dtype=torch.float32, device=ref.device)
        if B == 0:
            return out
        lib = _native.load()
        with torch.cuda.device(ref.device):
            _native.check(lib.escx_sisdr_metric(ref.data_ptr(), est.data_ptr(), B, L, lens, int(bool(self.scaling)), int(bool(self.zero_mean)), out.data_ptr(),
                                                _stream(ref.device)))
        return out


class EntropyCounter:
    """Counter maintaining codebook utilisation on a held-out set (metrics.py:12-77), on integer counts kept on the device.

    `update` takes the codes of a mixed-length batch as they come: the -1 filler past a clip's own frames is skipped, and the number of live
    frames (counted in one (stream, group) slot; every slot must have as many) is added to `total_counts`.  Equal counts give the rate and
    the dictionary of `scripts.metrics.EntropyCounter`: compute_utilization is its arithmetic."""

    def __init__(self, codebook_size=1024, num_streams=6, num_groups=3, device="cuda"):
        self.num_groups, self.codebook_size, self.device = num_groups, codebook_size, device
        self.reset_stats(num_streams)

    def reset_stats(self, num_streams):
        self.counts = torch.zeros(num_streams, self.num_groups, self.codebook_size, device=self.device, dtype=torch.int64)
        self._overflow = torch.zeros(1, device=self.device, dtype=torch.int64)
        self.total_counts = 0
        self.num_streams = num_streams
        self.max_entropy_per_book = math.log2(self.codebook_size)
        self.max_total_entropy = num_streams * self.num_groups * self.max_entropy_per_book

    def update(self, codes: torch.Tensor):
        if not isinstance(codes, torch.Tensor) or codes.dim() != 4 or codes.dtype.is_floating_point or codes.dtype.is_complex or codes.dtype == torch.bool:
            raise ValueError("codes must be an integer tensor of shape (B, num_streams, num_groups, T)")
        if codes.size(1) != self.num_streams or codes.size(2) != self.num_groups:
            raise ValueError(f"code indices size not match: codes {tuple(codes.shape)} for {self.num_streams} streams of {self.num_groups} groups")
        B, S, G, T = codes.shape
        live = (codes >= 0).sum(dim=(0, 3)).reshape(-1).tolist()
        if any(n != live[0] for n in live):
            raise ValueError(f"the (stream, group) slots hold different numbers of live frames ({sorted(set(live))}): per-clip bitrates are not counted here")
        _need_gpu(codes, "codes"); _need_gpu(self.counts, "the counter")
        codes = codes.to(device=self.counts.device, dtype=torch.int64).contiguous()
        if B == 0 or T == 0:
            return
        lib = _native.load()
        with torch.cuda.device(codes.device):
            _native.check(lib.escx_code_histogram(codes.data_ptr(), B, S, G, T, self.codebook_size, self.counts.data_ptr(), self._overflow.data_ptr(),
                                                  _stream(codes.device)))
        over = int(self._overflow.item())
        if over:
            self._overflow.zero_()
            raise ValueError(f"{over} codes at or above codebook_size={self.codebook_size}: they were not counted (call reset_stats before counting again)")
        self.total_counts += live[0]

    def compute_utilization(self):
        assert self.total_counts > 0, "No data collected, please update on a specific dataset"
        dist = (self.counts.to(torch.float64) / self.total_counts).to(torch.float32)
        ent = -(dist * torch.log2(dist + 1e-10)).sum(-1)               # (S, G)
        util = {f"stream_{s}_group_{g + 1}": round(float(ent[s, g]) / self.max_entropy_per_book, 4)
                for s in range(self.num_streams) for g in range(self.num_groups)}
        return round(float(ent.sum()) / self.max_total_entropy, 4), util
