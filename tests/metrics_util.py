"""Inputs and references of the length-aware metric tests (test_metrics_native_host.py on the host, test_metrics_native.py on the GPU).

The yardstick is the reference's per-clip semantics: the `scripts.metrics` classes (pinned to the real reference by tests/golden/metrics.npz) applied
in float64 to x[b, :L_b] and y[b, :L_b] alone.  The float32 run of the same classes is the comparison error.  Everything here runs on the CPU and is
computed once per process (functools.lru_cache); callers must not modify what they get.
"""
import functools
import os
import sys

import numpy as np
import torch

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
from scripts import metrics as M  # noqa: E402

import loss_util as LU  # noqa: E402

MEL_N = 4100                                                            # n_samples of the ragged mel batches
# the minimum length; both sides of a hop boundary at the 8-sample hop (1031 // 8 = 128, 1032 // 8 = 129); a clip with several dead 64-row tiles that ends
# inside a tile shared with dead rows (1025 samples: 129 of 513 frames at hop 8)
MEL_RAGGED_LENGTHS = ([4100, 1025, 2048], [1031, 1032, 4099], [2049, 4100, 1025])
MEL_UNIFORM = [(B, L) for L in LU.MEL_LENGTHS for B in (1, 3)]
MEL_KIND, MEL_GAIN = "noise", "step"                                    # loss_util.mel_case: both signs of the log difference, far from the clamp

SISDR_N = 4097
SISDR_LENGTHS = [2, 63, 64, 65, 257, 4097]                              # below / at / above one wave, one workgroup stride + 1, every sample
SISDR_MODES = ((True, True), (False, True), (True, False), (False, False))      # (scaling, zero_mean)

HIST_SHAPES = ((1, 1, 1, 1, 4), (3, 6, 3, 17, 1024), (2, 18, 1, 300, 1024))     # (B, S, G, T, K)


@functools.lru_cache(maxsize=None)
def _mel_modules():
    return M.MelSpectrogramDistance().double(), M.MelSpectrogramDistance()


@functools.lru_cache(maxsize=None)
def mel_pair(B, L):
    """(raw, rec) float32 (B, L) of loss_util.mel_case."""
    return LU.mel_case(MEL_KIND, MEL_GAIN, B, L)


def mel_clip_reference(x, y):
    """(float64 value, float32 value) of scripts.metrics.MelSpectrogramDistance on one clip (1-D tensors)."""
    d64, d32 = _mel_modules()
    with torch.no_grad():
        return float(d64(x[None].double(), y[None].double())[0]), float(d32(x[None].float(), y[None].float())[0])


@functools.lru_cache(maxsize=None)
def mel_reference(B, L, lengths=None):
    """float64 and float32 per-clip values (two (B,) arrays) of mel_pair(B, L) with clip b cut to lengths[b] (a tuple; None: whole clips)."""
    x, y = mel_pair(B, L)
    lens = [L] * B if lengths is None else list(lengths)
    vals = [mel_clip_reference(x[b, :n], y[b, :n]) for b, n in enumerate(lens)]
    return np.array([v[0] for v in vals]), np.array([v[1] for v in vals])


@functools.lru_cache(maxsize=None)
def sisdr_pair():
    g = torch.Generator().manual_seed(4097)
    x = 0.1 * torch.randn(len(SISDR_LENGTHS), SISDR_N, generator=g) + 0.02         # an offset: zero_mean matters
    y = 0.8 * x + 0.03 * torch.randn(len(SISDR_LENGTHS), SISDR_N, generator=g) - 0.01
    return x, y


@functools.lru_cache(maxsize=None)
def sisdr_reference(scaling, zero_mean):
    """float64 scripts.metrics.SISDR of every clip of sisdr_pair() cut to its length."""
    x, y = sisdr_pair()
    fn = M.SISDR(scaling=scaling, zero_mean=zero_mean)
    return np.array([float(fn(x[b:b + 1, :n].double(), y[b:b + 1, :n].double())[0]) for b, n in enumerate(SISDR_LENGTHS)])


def poison(t, lengths):
    """A copy of (B, L) `t` with NaN from lengths[b] on."""
    t = t.clone()
    for b, n in enumerate(lengths):
        t[b, n:] = float("nan")
    return t


@functools.lru_cache(maxsize=None)
def hist_codes(shape):
    """(codes (B, S, G, T) int64 with -1 tails, live frames per clip): clip b keeps T - (5 b) % T frames (all of them for clip 0)."""
    B, S, G, T, K = shape
    g = torch.Generator().manual_seed(31 * T + K)
    codes = torch.randint(0, K, (B, S, G, T), generator=g)
    codes[..., 0] = K - 1                                               # the last bin is hit
    live = [T - (5 * b) % T for b in range(B)]
    for b, n in enumerate(live):
        codes[b, :, :, n:] = -1
    return codes, live


def hist_reference(shape, repeats=1):
    """(counts (S, G, K) int64 by torch.bincount on the live codes, rate and dictionary of scripts.metrics.EntropyCounter fed clip by clip), the set fed `repeats` times."""
    B, S, G, T, K = shape
    codes, live = hist_codes(shape)
    counts = torch.zeros(S, G, K, dtype=torch.int64)
    ec = M.EntropyCounter(K, num_streams=S, num_groups=G, device="cpu")
    for _ in range(repeats):
        for b, n in enumerate(live):
            ec.update(codes[b:b + 1, :, :, :n])
            for s in range(S):
                for gg in range(G):
                    counts[s, gg] += torch.bincount(codes[b, s, gg, :n], minlength=K)
    return counts, ec.compute_utilization()


# ---- the harness -----------------------------------------------------------------------------------------
# Clips of the ESC harness test (tiny configuration): (kind, esc.synth tag, samples in the file).  On the CPU oracle the smallest argmin margin over
# all three streams at the snapped length is 4.0e-4, 1.5e-4, 9.1e-5, 7.2e-5 (test_metrics_native_host.py re-measures them): at least 35 x gpu_util.NEAR_TIE.
ESC_CLIPS = (("voiced", "ragged-eval-voiced-1", 4800), ("noise", "ragged-eval-noise-3", 7013), ("voiced", "ragged-eval-voiced-0", 11111),
             ("noise", "ragged-eval-noise-3", 16000))
ESC_MIN_MARGIN = 1e-5                                                   # 5 x NEAR_TIE
DAC_CLIPS = (("voiced", "ragged-dac-0", 4800), ("noise", "ragged-dac-1", 9999), ("voiced", "ragged-dac-2", 12345), ("noise", "ragged-dac-3", 16000))    # 0.3 .. 1.0 s


def clip_pcm(kind, tag, n):
    from esc import synth
    return (synth.voiced_clip_int16 if kind == "voiced" else synth.noise_clip_int16)(tag, n)


def write_wavs(folder, clips):
    """One 16 kHz wav per clip, named so that the name order is the order of `clips` (which is NOT the length order of the batches)."""
    from scipy.io import wavfile
    os.makedirs(folder, exist_ok=True)
    for i, (kind, tag, n) in enumerate(clips):
        wavfile.write(os.path.join(folder, f"clip{i}.wav"), 16000, clip_pcm(kind, tag, n))
    return folder
