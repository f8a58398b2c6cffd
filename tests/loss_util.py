"""Inputs and references of the loss-kernel tests (test_losses_host.py on the host, test_losses.py on the GPU).

Everything here runs on the CPU.  The builders are deterministic (seeded torch.Generator); the references evaluate the oracle's restatement of
generator_loss.py / gan_loss.py in float64 (the truth the kernels are held to) and in float32 (what the reference itself would give: its distance
from float64 is the yardstick of the harmonic-clip bound and the condition test_losses_host.py checks for every other case).

Why the gradient cases use SCALED reconstructions (rec = gain * raw) and not raw + noise: the mel loss is an L1 of mel values and of their logs, so its
gradient is a sum of signs.  With independent noise some cells of the two mel spectrograms nearly tie, float32 rounding flips their sign, and the
reference's OWN float32 gradient is then 1e-4 .. 2e-2 from float64 - a test built on that can neither pass tightly nor detect anything.  A gain keeps
every cell a fixed ratio apart (no ties) while the STFTs, filterbanks, clamps and the framing adjoint still see real signals; the step gain brings
both signs in.  tie_margins() measures the distance from a tie and test_losses_host.py asserts it, so a changed seed cannot quietly undo this.
"""
import math

import numpy as np
import torch

from oracle import esc_oracle as O

LOSS_RTOL = 1e-5        # tests/test_train.py
GRAD_TOL = 1e-4         # tests/test_train.py (relative RMS)
TIE_MARGIN = 1e-5       # 100 x the 1e-7 relative rounding of a float32 mel value
CLAMP_EPS = 1e-5        # generator_loss.py:56 clamp_eps
SR = 16000


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


# ---- clips ------------------------------------------------------------------------------------------
def noise_clip(B, L, seed, amp=0.1):
    return amp * torch.randn(B, L, generator=_gen(seed))


def harmonic_clip(B, L, seed):
    """0.3 * sum_{k<6} 0.5^k sin(2 pi 200 (k+1) t + k) at 16 kHz plus a 1e-4 noise floor (the floor differs per clip): near-empty mel bins between the partials."""
    t = torch.arange(L, dtype=torch.float64) / SR
    h = sum(0.5 ** k * torch.sin(2 * math.pi * 200.0 * (k + 1) * t + k) for k in range(6))
    return (0.3 * h).float().unsqueeze(0).repeat(B, 1) + 1e-4 * torch.randn(B, L, generator=_gen(seed))


def quiet_clip(B, L, seed):
    return noise_clip(B, L, seed, amp=1e-4)


def silent_clip(B, L):
    return torch.zeros(B, L)


def make_clip(kind, B, L, seed):
    if kind == "noise":
        return noise_clip(B, L, seed)
    if kind == "harmonic":
        return harmonic_clip(B, L, seed)
    if kind == "quiet":
        return quiet_clip(B, L, seed)
    if kind == "at_clamp":          # mel values on both sides of clamp_eps at several resolutions
        return noise_clip(B, L, seed, amp=1e-5)
    if kind == "below_clamp":
        return noise_clip(B, L, seed, amp=1e-8)
    if kind == "silent":
        return silent_clip(B, L)
    raise KeyError(kind)


GAINS = ("half", "up", "step")


def apply_gain(raw, gain):
    """rec = gain * raw in float32: constant 0.5, constant 1.7, or 0.5 on the first half of the clip and 1.7 on the second."""
    L = raw.shape[-1]
    if gain == "half":
        return 0.5 * raw
    if gain == "up":
        return 1.7 * raw
    if gain == "step":
        g = torch.full((L,), 0.5)
        g[L // 2:] = 1.7
        return raw * g
    raise KeyError(gain)


def mel_case(kind, gain, B, L, seed=None):
    """(raw, rec) float32 (B, L) of one mel-loss case; the seed follows from the case unless given."""
    if seed is None:
        seed = 1000 + 7 * L + 13 * B + {"noise": 0, "harmonic": 1, "quiet": 2, "below_clamp": 3, "silent": 4, "at_clamp": 5}[kind]
    raw = make_clip(kind, B, L, seed)
    return raw, apply_gain(raw, gain)


# ---- the mel loss -----------------------------------------------------------------------------------
def mel_loss_at_rate(raw, rec, sample_rate=SR, clamp_eps=CLAMP_EPS):
    """O.mel_spectrogram_loss with the sample rate passed through to the filterbanks (the oracle's own loss fixes 16000)."""
    loss = 0.0
    for w, nm in zip(O.MEL_WINDOWS, O.MEL_BINS):
        xm, ym = O.mel_spectrogram(raw, w, nm, sample_rate=sample_rate), O.mel_spectrogram(rec, w, nm, sample_rate=sample_rate)
        loss = loss + (xm - ym).abs().mean([1, 2])
        loss = loss + (xm.clamp(clamp_eps).pow(2).log10() - ym.clamp(clamp_eps).pow(2).log10()).abs().mean([1, 2])
    return loss


def _with_grads(fn, a, b, dtype, weights=None):
    a = a.detach().to(dtype).requires_grad_(True)
    b = b.detach().to(dtype).requires_grad_(True)
    loss = fn(a, b)
    w = torch.ones_like(loss) if weights is None else torch.as_tensor(weights).to(dtype)
    (loss * w).sum().backward()
    return (loss.detach().double().numpy(), a.grad.double().numpy(), b.grad.double().numpy())


def mel_reference(raw, rec, dtype=torch.float64, sample_rate=SR, weights=None):
    """(loss (B,), d sum_b w_b loss_b / d raw, d .. / d rec) as float64 arrays, evaluated in `dtype`."""
    if sample_rate == SR:
        return _with_grads(O.mel_spectrogram_loss, raw, rec, dtype, weights)
    return _with_grads(lambda a, b: mel_loss_at_rate(a, b, sample_rate), raw, rec, dtype, weights)


def stft_reference(raw, rec, dtype=torch.float64, weights=None):
    """The same for O.complex_stft_loss on flat (B, per_clip) buffers (the loss is a mean over everything but the batch)."""
    fn = lambda a, b: O.complex_stft_loss(a.reshape(a.shape[0], 1, 1, -1), b.reshape(b.shape[0], 1, 1, -1))
    return _with_grads(fn, raw, rec, dtype, weights)


def tie_margins(raw, rec, sample_rate=SR):
    """Distance of a mel-loss input from the points where its gradient jumps, in float64 over the seven resolutions:
    (min |x - y| / (x + y),  min |lx - ly| over cells where either side is above the clamp,  min |v - clamp| / clamp over both sides).
    Cells where both mels are exactly 0 (two silent frames) carry no gradient and are left out of the first measure."""
    lin, log, clamp = math.inf, math.inf, math.inf
    raw, rec = raw.double(), rec.double()
    for w, nm in zip(O.MEL_WINDOWS, O.MEL_BINS):
        x, y = O.mel_spectrogram(raw, w, nm, sample_rate=sample_rate), O.mel_spectrogram(rec, w, nm, sample_rate=sample_rate)
        live = (x + y) > 0
        if live.any():
            lin = min(lin, float(((x - y).abs()[live] / (x + y)[live]).min()))
        above = (x >= CLAMP_EPS) | (y >= CLAMP_EPS)
        if above.any():
            lx, ly = x.clamp(CLAMP_EPS).pow(2).log10(), y.clamp(CLAMP_EPS).pow(2).log10()
            log = min(log, float((lx - ly).abs()[above].min()))
        for v in (x, y):
            clamp = min(clamp, float(((v - CLAMP_EPS).abs() / CLAMP_EPS).min()))
    return lin, log, clamp


def clamp_straddles(raw, rec, sample_rate=SR):
    """(cells with rec < clamp <= raw, cells with raw < clamp <= rec) over the seven resolutions, in float64: where exactly one side's log gradient is cut by the clamp."""
    n_rec, n_raw = 0, 0
    raw, rec = raw.double(), rec.double()
    for w, nm in zip(O.MEL_WINDOWS, O.MEL_BINS):
        x, y = O.mel_spectrogram(raw, w, nm, sample_rate=sample_rate), O.mel_spectrogram(rec, w, nm, sample_rate=sample_rate)
        n_rec += int(((y < CLAMP_EPS) & (x >= CLAMP_EPS)).sum())
        n_raw += int(((x < CLAMP_EPS) & (y >= CLAMP_EPS)).sum())
    return n_rec, n_raw


def rel_rms(a, b, floor=1e-30):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(float(np.sqrt(np.mean(b ** 2))), floor))


def rel_err(a, b):
    """Worst relative error of a vector of per-clip losses."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


# The well-conditioned mel cases of test_losses.py: (kind, gain, B, L).  test_losses_host.py checks every one of them.
MEL_LENGTHS = (1025, 1026, 2047, 2048, 2049, 4100)
MEL_WELL = ([("noise", g, B, L) for L in MEL_LENGTHS for B in (1, 3) for g in GAINS]
            + [("quiet", "half", B, L) for L in MEL_LENGTHS for B in (1, 3)]
            + [("at_clamp", g, 2, 2049) for g in ("half", "up")])
MEL_AT_CLAMP_MIN_CELLS = 20         # cells with one side clamped and the other not that an at_clamp case must have (x 0.5: recon side clamped, x 1.7: raw side clamped)
# 65 clips x step gain do produce a near-tie (2e-7): a constant gain here.  Among 65 noise clips one usually has a mel cell that is nearly empty by chance, where the
# log term's 1 / y amplifies the float32 rounding of y: the float32 oracle's own gradient is then 0.8 .. 5.7e-4 from float64 (seeds 11-16 tried).  Seed 15 has none (7e-6).
MEL_WELL_B65 = ("noise", "up", 65, 1025)
MEL_WELL_B65_SEED = 15
MEL_BELOW_CLAMP = ("below_clamp", "half", 2, 2049)
MEL_HARMONIC = [("harmonic", g, 2, L) for L in (1025, 2049, 6000) for g in ("half", "up")]
MEL_MODULE = ("noise", "step", 3, 2049)
MEL_MODULE_WEIGHTS = (0.5, 1.0, -2.0)
MEL_RATE = ("noise", "half", 2, 2049)


# ---- the STFT loss ----------------------------------------------------------------------------------
STFT_SIZES = (1, 255, 256, 257, 16384, 16385, 40000)
STFT_CASES = [(B, n) for n in STFT_SIZES for B in (1, 2)] + [(65, 257)]


def stft_case(B, per_clip, seed=None):
    """(raw, rec, planted) float32 (B, per_clip): noise with planted exact zeros, +-1e-12, a 3e3 and sign changes on BOTH sides, at the head and at the tail
    of every clip (the tail lies in the second grid-stride trip when per_clip > 16384).  planted: bool mask of the touched positions."""
    g = _gen(2000 + 3 * per_clip + B if seed is None else seed)
    raw = torch.randn(B, per_clip, generator=g)
    rec = raw + 0.3 * torch.randn(B, per_clip, generator=g)
    planted = torch.zeros(B, per_clip, dtype=torch.bool)
    if per_clip == 1:       # one element per clip: clip 0 has a zero on the recon side, clip 1 opposite signs (both far from a cancellation in pl(a) - pl(r))
        raw[0, 0], rec[0, 0] = 0.7, 0.0
        if B > 1:
            raw[1, 0], rec[1, 0] = -0.9, 0.6
        planted[:] = True
        return raw, rec, planted
    plants = [(None, 0.0), (0.0, None), (0.0, 0.0), (None, 1e-12), (None, -1e-12), (1e-12, None), (-1e-12, None), (1e-12, -1e-12), (None, 3e3), (-3e3, None),
              (0.0, 1e-12), (-1e-12, 0.0)]            # (raw, rec); None = keep the noise
    for b in range(B):
        for k, (a, r) in enumerate(plants):
            for pos in ((17 * k + 5 * b) % per_clip, per_clip - 1 - (13 * k + 3 * b) % per_clip):
                if a is not None:
                    raw[b, pos] = a
                if r is not None:
                    rec[b, pos] = r
                planted[b, pos] = True
    return raw, rec, planted


# ---- GAN terms --------------------------------------------------------------------------------------
GAN_GEOMETRIES = ((1, 4, 7, 3, 3), (30, 32, 5, 9, 9), (32, 32, 4, 6, 11), (128, 128, 9, 60, 60), (3, 4, 1, 1, 1))       # (C, Cp, D0, D1, P1)
GAN_CASES = [(geo, B) for geo in GAN_GEOMETRIES for B in (1, 3)] + [(GAN_GEOMETRIES[0], 65)]


def gan_case(geo, B, seed=None):
    """Logical (B, C, D0, D1) float32 maps x and ref; ref equals x exactly at a few planted elements of every clip."""
    C, Cp, D0, D1, P1 = geo
    g = _gen(3000 + 31 * C + 7 * D0 * D1 + B if seed is None else seed)
    x = torch.randn(B, C, D0, D1, generator=g)
    ref = x + 0.5 * torch.randn(B, C, D0, D1, generator=g)
    same = torch.zeros(B, C, D0, D1, dtype=torch.bool)
    n = C * D0 * D1
    flat_same = same.view(B, n)
    for b in range(B):
        for k in range(min(5, max(1, n // 3))):
            flat_same[b, (11 * k + b) % n] = True
        flat_same[b, n - 1] = n > 1
    ref = torch.where(same, x, ref)
    return x, ref, same


def gan_reference(x, ref, mode, target=0.0, g=None):
    """float64: per-clip loss (B,) and d (sum_b g_b loss_b) / d x on the logical (B, C, D0, D1) map; mode 0 = mean (target - x)^2, mode 1 = mean |x - ref|."""
    x64 = x.double()
    n = x64[0].numel()
    gb = torch.ones(x.shape[0], dtype=torch.float64) if g is None else torch.as_tensor(g).double()
    gb = gb.view(-1, 1, 1, 1)
    if mode == 0:
        d = target - x64
        return (d * d).mean([1, 2, 3]).numpy(), (-2.0 * d * gb / n).numpy()
    d = x64 - ref.double()
    return d.abs().mean([1, 2, 3]).numpy(), (torch.sign(d) * gb / n).numpy()


def gan_pack(x, Cp, P1, fill=0.0):
    """Logical (B, C, D0, D1) -> the channels-last (B, D0, P1, Cp) buffer the kernel takes; pad channels and the pitch-gap columns D1..P1 hold `fill`."""
    B, C, D0, D1 = x.shape
    assert C <= Cp and D1 <= P1
    buf = torch.full((B, D0, P1, Cp), float(fill), dtype=x.dtype)
    buf[:, :, :D1, :C] = x.permute(0, 2, 3, 1)
    return buf


def gan_unpack(buf, C, D1):
    """The logical (B, C, D0, D1) map of a (B, D0, P1, Cp) buffer."""
    return buf[:, :, :D1, :C].permute(0, 3, 1, 2).contiguous()


# ---- flat optimiser ---------------------------------------------------------------------------------
def clip_adamw_reference(p0, grads, max_norm, lr, beta1, beta2, eps, weight_decay):
    """float64 restatement of torch.nn.utils.clip_grad_norm_(max_norm) + torch.optim.AdamW.step() on one flat tensor.  Yields (norm, parameters) after every step."""
    p = p0.double().clone(); m = torch.zeros_like(p); v = torch.zeros_like(p)
    for t, g in enumerate(grads, 1):
        g = g.double()
        norm = float(g.pow(2).sum().sqrt())
        g = g * min(1.0, max_norm / (norm + 1e-6))
        p = p * (1.0 - lr * weight_decay)
        m = beta1 * m + (1.0 - beta1) * g
        v = beta2 * v + (1.0 - beta2) * g * g
        bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
        p = p - (lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
        yield norm, p.clone()
