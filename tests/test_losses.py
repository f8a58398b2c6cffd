"""The hand-written loss kernels at their edges, against float64.

Every training step ends in escx_stft_loss[_ex], escx_mel_loss[_ex], escx_gan_term[_grad] and escx_scale_rows, and their gradients seed the whole backward
pass.  These tests call them through the C entry points (and once each through the modules) and hold them to the float64 evaluation of the oracle's
restatement: LOSS_RTOL on the per-clip loss, GRAD_TOL (relative RMS) on both gradients, the project's constants of tests/test_train.py.  The inputs come
from loss_util.py; test_losses_host.py proves on the host that every case bounded this way is well conditioned (no L1 tie, no cell at the clamp, the float32
oracle itself inside the tolerances).  The harmonic clip is the exception: there the float32 oracle's own gradient is 2..4e-4 from float64 (the log term's
1 / y in near-empty mel bins), so the device is held to max(GRAD_TOL, 3 x that), the form of bound tests/test_msd.py uses.

Every case prints device error, float32-oracle error and their ratio ("[loss-edges] ..."); profiles/loss_edges.txt is that printout of one run.

Branch / trip -> test:
  stft_loss_kernel second grid-stride trip (per_clip > 16384) ............ test_stft_loss_sizes_and_planted_values[*-16385], [*-40000]
  row_sum_kernel second block (B > 64) ................................... test_stft_loss_sizes_and_planted_values[65-257], test_mel_loss_65_clips, test_gan_terms[1x4x7x3x3-65]
  sign(0) kills a term on the recon side, |x| < eps ...................... test_stft_loss_sizes_and_planted_values (planted 0, +-1e-12 on both sides)
  L = 1025: both mirrors of frames_bwd_kernel on one sample .............. test_mel_loss_well_conditioned[*-1025]
  Tm = 1 + L / hop roundings, pad columns Fq > F and Mp > n_mels ......... test_mel_loss_well_conditioned (L = 1026, 2047, 2048, 2049, 4100; all seven resolutions)
  mel_l1_kernel clamp branches ........................................... test_mel_loss_well_conditioned[at_clamp-half-2-2049] (recon side), [at_clamp-up-2-2049] (raw side),
                                                                           test_mel_loss_below_clamp (both sides clamped: the log term vanishes)
  complex_mag_bwd_kernel m > 0 ........................................... test_mel_loss_one_side_silent, test_mel_loss_both_sides_silent
  stream_scratch arena reuse across calls ................................ test_mel_scratch_reuse_across_calls
  build_mel rebuild on a sample-rate change .............................. test_mel_sample_rate_switch_rebuilds_the_tables
  gan_term_kernel C < Cp, P1 > D1, per4 > 16384, accumulate, x == ref .... test_gan_terms
  sumsq_partial_kernel second grid-stride trip (n > 262144) .............. test_flat_optimiser_sizes[262401]
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import loss_util as U
from loss_util import GRAD_TOL, LOSS_RTOL

pytestmark = pytest.mark.gpu

HARMONIC_FACTOR = 3.0           # tests/test_msd.py: device error <= max(absolute tolerance, 3 x the float32 restatement's own error)


def _lib():
    from esc import _native
    return _native.load()


def _p(t, offset=0):
    return None if t is None else ctypes.c_void_p(t.data_ptr() + offset)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(rc):
    from esc import _native
    _native.check(rc)


def _nan_like(t):
    return torch.full_like(t, float("nan"))


def _ratio(dev, ref):
    return dev / max(ref, 1e-30)


def _report(tag, dev, ref):
    """dev / ref: (loss, d_raw, d_rec) errors of the device and of the float32 oracle, both against float64."""
    parts = [f"{n} device {d:.2e} float32 {r:.2e} ratio {_ratio(d, r):.2f}" for n, d, r in zip(("loss", "d_raw", "d_rec"), dev, ref)]
    print(f"[loss-edges] {tag}: " + "   ".join(parts))


# ---- ComplexSTFTLoss ----------------------------------------------------------------------------------
def _run_stft(raw, rec, want_raw=True, ex=True):
    lib = _lib()
    B, per = raw.shape
    r, c = raw.cuda().contiguous(), rec.cuda().contiguous()
    loss = torch.full((B,), float("nan"), device="cuda")
    d_rec, d_raw = _nan_like(c), (_nan_like(r) if want_raw else None)
    if ex:
        _check(lib.escx_stft_loss_ex(_p(r), _p(c), B, per, _p(loss), _p(d_rec), _p(d_raw), _stream()))
    else:
        _check(lib.escx_stft_loss(_p(r), _p(c), B, per, _p(loss), _p(d_rec), _stream()))
    torch.cuda.synchronize()
    return loss.cpu(), (None if d_raw is None else d_raw.cpu()), d_rec.cpu()


@pytest.mark.parametrize("B,per_clip", U.STFT_CASES)
def test_stft_loss_sizes_and_planted_values(B, per_clip):
    """escx_stft_loss_ex on flat (B, per_clip) buffers: one element, around the 256-element block, around the 16384-element grid (the second grid-stride trip of
    stft_loss_kernel) and 65 clips (the second block of row_sum_kernel), with exact zeros, +-1e-12 (below the power law's eps), a 3e3 and sign changes planted on
    BOTH sides, also where both sides are zero.  Loss within LOSS_RTOL and both gradients within GRAD_TOL of float64 - over everything and over the unplanted
    elements alone, which the huge gradients at +-1e-12 would otherwise hide; a gradient is exactly 0 where its own input is exactly 0; escx_stft_loss writes
    bitwise the d_recon of escx_stft_loss_ex."""
    raw, rec, planted = U.stft_case(B, per_clip)
    l64, a64, b64 = U.stft_reference(raw, rec, torch.float64)
    l32, a32, b32 = U.stft_reference(raw, rec, torch.float32)
    loss, d_raw, d_rec = _run_stft(raw, rec)
    assert torch.isfinite(loss).all() and torch.isfinite(d_raw).all() and torch.isfinite(d_rec).all()
    dev = (U.rel_err(loss, l64), U.rel_rms(d_raw, a64), U.rel_rms(d_rec, b64))
    _report(f"stft B={B} per_clip={per_clip}", dev, (U.rel_err(l32, l64), U.rel_rms(a32, a64), U.rel_rms(b32, b64)))
    assert dev[0] <= LOSS_RTOL and dev[1] <= GRAD_TOL and dev[2] <= GRAD_TOL, dev
    keep = ~planted.numpy()
    if keep.any():
        rest = (U.rel_rms(d_raw.numpy()[keep], a64[keep]), U.rel_rms(d_rec.numpy()[keep], b64[keep]))
        print(f"[loss-edges] stft B={B} per_clip={per_clip} unplanted elements: d_raw device {rest[0]:.2e}   d_rec device {rest[1]:.2e}")
        assert max(rest) <= GRAD_TOL, rest
    assert bool((d_rec[rec == 0] == 0).all()) and bool((d_raw[raw == 0] == 0).all())
    loss1, _, d_rec1 = _run_stft(raw, rec, want_raw=False, ex=False)
    assert torch.equal(loss1, loss) and torch.equal(d_rec1, d_rec)


@pytest.mark.parametrize("B,F,T", [(2, 8, 16), (2, 64, 128), (1, 100, 200)])
def test_stft_loss_module_with_unequal_weights(B, F, T):
    """ComplexSTFTLoss on (B, 2, F, T) with both arguments differentiable and unequal per-clip upstream gradients (escx_scale_rows): the module returns what the
    entry point returns on the flat buffers, and the gradients are the float64 reference's."""
    from esc.modules import ComplexSTFTLoss
    raw, rec, _ = U.stft_case(B, 2 * F * T)
    w = torch.tensor([0.5, -2.0][:B])
    l64, a64, b64 = U.stft_reference(raw, rec, torch.float64, weights=w)
    ra = raw.view(B, 2, F, T).cuda().requires_grad_(True)
    rc = rec.view(B, 2, F, T).cuda().requires_grad_(True)
    got = ComplexSTFTLoss()(ra, rc)
    (got * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    loss, _, _ = _run_stft(raw, rec)
    assert torch.equal(got.detach().cpu(), loss)
    dev = (U.rel_err(got.detach().cpu(), l64), U.rel_rms(ra.grad.cpu().reshape(B, -1), a64), U.rel_rms(rc.grad.cpu().reshape(B, -1), b64))
    print(f"[loss-edges] stft module B={B} F={F} T={T}: loss {dev[0]:.2e}   d_raw {dev[1]:.2e}   d_rec {dev[2]:.2e}")
    assert dev[0] <= LOSS_RTOL and dev[1] <= GRAD_TOL and dev[2] <= GRAD_TOL, dev


@pytest.mark.parametrize("per_clip", [257, 40000])
def test_stft_loss_of_identical_inputs_is_exactly_zero(per_clip):
    """recon == raw bitwise (planted values included): loss exactly 0, both gradients exactly 0."""
    raw, _, _ = U.stft_case(2, per_clip)
    loss, d_raw, d_rec = _run_stft(raw, raw.clone())
    assert bool((loss == 0).all()) and bool((d_raw == 0).all()) and bool((d_rec == 0).all())


# ---- MelSpectrogramLoss -------------------------------------------------------------------------------
def _run_mel(raw, rec, sample_rate=U.SR, want_raw=True, want_rec=True):
    lib = _lib()
    B, L = raw.shape
    r, c = raw.cuda().contiguous(), rec.cuda().contiguous()
    loss = torch.full((B,), float("nan"), device="cuda")
    d_rec, d_raw = (_nan_like(c) if want_rec else None), (_nan_like(r) if want_raw else None)
    _check(lib.escx_mel_loss_ex(_p(r), _p(c), B, L, sample_rate, _p(loss), _p(d_rec), _p(d_raw), _stream()))
    torch.cuda.synchronize()
    return loss.cpu(), (None if d_raw is None else d_raw.cpu()), (None if d_rec is None else d_rec.cpu())


@functools.lru_cache(maxsize=None)
def _mel_refs(kind, gain, B, L, seed=None):
    """(raw, rec, float64 reference, float32 reference) of one case, computed once."""
    raw, rec = U.mel_case(kind, gain, B, L, seed)
    return raw, rec, U.mel_reference(raw, rec, torch.float64), U.mel_reference(raw, rec, torch.float32)


def _mel_errors(got, ref64):
    loss, d_raw, d_rec = got
    assert torch.isfinite(loss).all() and torch.isfinite(d_raw).all() and torch.isfinite(d_rec).all()
    return U.rel_err(loss, ref64[0]), U.rel_rms(d_raw, ref64[1]), U.rel_rms(d_rec, ref64[2])


def _mel_bounded(tag, raw, rec, ref64, ref32, sample_rate=U.SR):
    dev = _mel_errors(_run_mel(raw, rec, sample_rate), ref64)
    _report(tag, dev, (U.rel_err(ref32[0], ref64[0]), U.rel_rms(ref32[1], ref64[1]), U.rel_rms(ref32[2], ref64[2])))
    assert dev[0] <= LOSS_RTOL, f"{tag}: loss {dev[0]:.3e} from float64"
    assert dev[1] <= GRAD_TOL and dev[2] <= GRAD_TOL, f"{tag}: gradients {dev[1]:.3e} (raw) / {dev[2]:.3e} (recon) from float64"


@pytest.mark.parametrize("kind,gain,B,L", U.MEL_WELL, ids=lambda v: str(v))
def test_mel_loss_well_conditioned(kind, gain, B, L):
    """escx_mel_loss_ex with both unit gradients on noise x {0.5, 1.7, step gain} and the quiet clip x 0.5, plus the at_clamp clip (amplitude 1e-5: dozens of mel cells
    with one side below clamp_eps and the other above, the `>= clamp_eps` branches of mel_l1_kernel - the recon side's at gain 0.5, the raw side's at 1.7): L = 1025 (the shortest length the entry point takes: the left and
    the right mirror of frames_bwd_kernel fold onto the same samples), 1026, 2047, 2048 (every hop divides L), 2049, 4100 (none does) - so Tm = 1 + L / hop takes each of its
    roundings at the seven resolutions, with the pad columns Fq > F everywhere and Mp > n_mels at 5, 10, 20 and 40 bins.  Loss within LOSS_RTOL, both gradients within GRAD_TOL."""
    raw, rec, ref64, ref32 = _mel_refs(kind, gain, B, L)
    _mel_bounded(f"mel {kind} x {gain} B={B} L={L}", raw, rec, ref64, ref32)


def test_mel_loss_65_clips():
    """B = 65 at L = 1025: the second block of row_sum_kernel, and clip indices past 64 in every per-clip grid."""
    kind, gain, B, L = U.MEL_WELL_B65
    raw, rec, ref64, ref32 = _mel_refs(kind, gain, B, L, U.MEL_WELL_B65_SEED)
    _mel_bounded(f"mel {kind} x {gain} B={B} L={L}", raw, rec, ref64, ref32)


def test_mel_loss_module_with_unequal_weights():
    """MelSpectrogramLoss with both arguments differentiable and unequal (one negative) per-clip upstream gradients: escx_scale_rows on both sides."""
    from esc.modules import MelSpectrogramLoss
    kind, gain, B, L = U.MEL_MODULE
    raw, rec = U.mel_case(kind, gain, B, L)
    w = torch.tensor(U.MEL_MODULE_WEIGHTS)
    ref64 = U.mel_reference(raw, rec, torch.float64, weights=w)
    ra, rc = raw.cuda().requires_grad_(True), rec.cuda().requires_grad_(True)
    got = MelSpectrogramLoss()(ra, rc)
    (got * w.cuda()).sum().backward()
    torch.cuda.synchronize()
    dev = _mel_errors((got.detach().cpu(), ra.grad.cpu(), rc.grad.cpu()), ref64)
    print(f"[loss-edges] mel module {kind} x {gain} B={B} L={L} weights {U.MEL_MODULE_WEIGHTS}: loss {dev[0]:.2e}   d_raw {dev[1]:.2e}   d_rec {dev[2]:.2e}")
    assert dev[0] <= LOSS_RTOL and dev[1] <= GRAD_TOL and dev[2] <= GRAD_TOL, dev
    unit = _run_mel(raw, rec)
    for b in range(B):          # backward only scales the stored unit gradient: one float32 multiply per element
        assert torch.equal(rc.grad[b].cpu(), unit[2][b] * w[b]) and torch.equal(ra.grad[b].cpu(), unit[1][b] * w[b])


def test_scale_rows_edges():
    """escx_scale_rows with rows = 0 (no launch, nothing written), per_row = 1 and an odd shape: out[r][:] = x[r][:] * g[r], one float32 multiply."""
    lib = _lib()
    gen = torch.Generator().manual_seed(9)
    for rows, per_row in ((0, 5), (300, 1), (3, 1027), (2, 0)):
        x = torch.randn(max(rows, 1), max(per_row, 1), generator=gen); g = torch.randn(max(rows, 1), generator=gen)
        xd, gd = x.cuda(), g.cuda()
        out = torch.full_like(xd, -7.0)
        _check(lib.escx_scale_rows(_p(xd), _p(gd), _p(out), rows, per_row, _stream()))
        torch.cuda.synchronize()
        want = x * g[:, None] if rows and per_row else torch.full_like(x, -7.0)
        assert torch.equal(out.cpu(), want), (rows, per_row)
    from esc import _native
    assert lib.escx_scale_rows(_p(xd), _p(gd), _p(out), -1, 1, _stream()) == _native.ESCX_ERR_INVALID_ARG


@pytest.mark.parametrize("kind", ["noise", "harmonic"])
def test_mel_loss_of_identical_inputs_is_exactly_zero(kind):
    """recon == raw bitwise: both sides run the same kernels on the same numbers, so every mel cell ties exactly: loss exactly 0 and, sign(0) = 0, both gradients exactly 0."""
    raw = U.make_clip(kind, 2, 2049, 77)
    loss, d_raw, d_rec = _run_mel(raw, raw.clone())
    assert bool((loss == 0).all()) and bool((d_raw == 0).all()) and bool((d_rec == 0).all())


@pytest.mark.parametrize("silent", ["raw", "recon"])
def test_mel_loss_one_side_silent(silent):
    """One side all zeros, the other noise.  Every mel cell of the silent side sits below the clamp (no log gradient: the `>= clamp_eps` branches of mel_l1_kernel) and every
    |S| of it is exactly 0 (the `m > 0` branch of complex_mag_bwd_kernel): in float64 its gradient is exactly 0, and so it must be here.  Loss within LOSS_RTOL; the noise
    side's gradient within GRAD_TOL (test_losses_host.py: the case is well conditioned); everything finite."""
    noise, zeros = U.noise_clip(2, 2049, 41), U.silent_clip(2, 2049)
    raw, rec = (zeros, noise) if silent == "raw" else (noise, zeros)
    ref64, ref32 = U.mel_reference(raw, rec, torch.float64), U.mel_reference(raw, rec, torch.float32)
    got = _run_mel(raw, rec)
    dev = _mel_errors(got, ref64)
    _report(f"mel silent {silent} side B=2 L=2049", dev, (U.rel_err(ref32[0], ref64[0]), U.rel_rms(ref32[1], ref64[1]), U.rel_rms(ref32[2], ref64[2])))
    assert dev[0] <= LOSS_RTOL
    i = 1 if silent == "raw" else 2
    assert not ref64[i].any() and np.array_equal(got[i].numpy().astype(np.float64), ref64[i])
    assert dev[3 - i] <= GRAD_TOL, dev


def test_mel_loss_both_sides_silent():
    """Both sides all zeros: loss 0, gradients 0, no NaN from 0 / |S| or from the log of a clamped 0."""
    z = U.silent_clip(2, 1025)
    loss, d_raw, d_rec = _run_mel(z, z.clone())
    assert bool((loss == 0).all()) and bool((d_raw == 0).all()) and bool((d_rec == 0).all())


def test_mel_loss_below_clamp():
    """Amplitude 1e-8: every mel value of both sides lies below clamp_eps (asserted in test_losses_host.py), both logs clamp to the same constant, the log term is exactly 0
    and only the linear term survives - in the loss (LOSS_RTOL) and in both gradients (GRAD_TOL against float64).  Mel values of 1e-7 and gradients that are pure signs."""
    kind, gain, B, L = U.MEL_BELOW_CLAMP
    raw, rec, ref64, ref32 = _mel_refs(kind, gain, B, L)
    _mel_bounded(f"mel {kind} x {gain} B={B} L={L}", raw, rec, ref64, ref32)


@pytest.mark.parametrize("kind,gain,B,L", U.MEL_HARMONIC, ids=lambda v: str(v))
def test_mel_loss_harmonic_clip(kind, gain, B, L):
    """Six partials of 200 Hz over a 1e-4 noise floor, scaled reconstructions: no ties, a loss value as well conditioned as any (LOSS_RTOL), but near-empty mel bins between
    the partials where the log term's 1 / y amplifies the rounding of y.  The float32 oracle's own gradient is 2..4e-4 from float64 there, so the bound is relative:
    device error <= max(GRAD_TOL, 3 x the float32 oracle's error on the same input)."""
    raw, rec, ref64, ref32 = _mel_refs(kind, gain, B, L)
    dev = _mel_errors(_run_mel(raw, rec), ref64)
    ref = (U.rel_err(ref32[0], ref64[0]), U.rel_rms(ref32[1], ref64[1]), U.rel_rms(ref32[2], ref64[2]))
    _report(f"mel {kind} x {gain} B={B} L={L}", dev, ref)
    assert dev[0] <= LOSS_RTOL, f"loss {dev[0]:.3e} from float64"
    for name, d, r in (("d_raw", dev[1], ref[1]), ("d_rec", dev[2], ref[2])):
        assert d <= max(GRAD_TOL, HARMONIC_FACTOR * r), f"{name}: device {d:.3e} vs float32 oracle {r:.3e} (ratio {_ratio(d, r):.2f})"


@pytest.mark.parametrize("scale", [1.0, 1e3])
def test_mel_scratch_reuse_across_calls(scale):
    """One stream: (B=1, L=1025), then (B=3, L=6000) with the raw-side gradient (the arena grows and is reallocated), then the first call again in the grown arena that the
    big call has just filled - with the big call's inputs scaled by 1e3 in the second round, so that a stale value read by the small call would show.  First and third
    results are bitwise equal (loss, both gradients), and the big call in between is right."""
    small = U.mel_case("noise", "step", 1, 1025)
    raw, rec, ref64, _ = _mel_refs("noise", "step", 3, 6000)
    first = _run_mel(*small)
    big = _run_mel(raw * scale, rec * scale)
    third = _run_mel(*small)
    for a, b in zip(first, third):
        assert torch.equal(a, b)
    if scale == 1.0:
        dev = _mel_errors(big, ref64)
        print(f"[loss-edges] mel noise x step B=3 L=6000 (between two small calls): loss {dev[0]:.2e}   d_raw {dev[1]:.2e}   d_rec {dev[2]:.2e}")
        assert dev[0] <= LOSS_RTOL and dev[1] <= GRAD_TOL and dev[2] <= GRAD_TOL, dev
    else:
        assert all(bool(torch.isfinite(t).all()) for t in big)


def test_mel_sample_rate_switch_rebuilds_the_tables():
    """sample_rate 16000 -> 8000 -> 16000 through the C entry point: build_mel frees and rebuilds the per-device tables on each change.  First and third results bitwise
    equal; the 8000 result within LOSS_RTOL / GRAD_TOL of the float64 restatement evaluated at 8000 (and the 16000 one of the one at 16000)."""
    kind, gain, B, L = U.MEL_RATE
    raw, rec = U.mel_case(kind, gain, B, L)
    first = _run_mel(raw, rec, 16000)
    ref64, ref32 = U.mel_reference(raw, rec, torch.float64, 8000), U.mel_reference(raw, rec, torch.float32, 8000)
    _mel_bounded(f"mel at 8 kHz {kind} x {gain} B={B} L={L}", raw, rec, ref64, ref32, sample_rate=8000)
    third = _run_mel(raw, rec, 16000)
    for a, b in zip(first, third):
        assert torch.equal(a, b)
    dev = _mel_errors(third, U.mel_reference(raw, rec, torch.float64))
    assert dev[0] <= LOSS_RTOL and dev[1] <= GRAD_TOL and dev[2] <= GRAD_TOL, dev
    assert abs(float(first[0][0]) - float(ref64[0][0])) > 100 * LOSS_RTOL * float(ref64[0][0])          # the two rates do differ


def test_mel_loss_of_a_clip_does_not_depend_on_its_batch():
    """Clip b of a B = 3 call against the B = 1 call on that clip.  gemm_frames always takes 64-row tiles, but gemm_rows (fp32 engine and split-operand route alike) switches
    to 128-row tiles once ceil(M / 128) x column tiles >= 512, so in general the tile choice DOES depend on M = B x frames and bitwise equality across batch sizes is not the
    library's contract: each clip, alone and in the batch, is held to the float64 bounds.  At these sizes (M <= 3 x 513 rows, at most 17 column tiles: 13 x 17 < 512) both calls
    stay on 64-row tiles, where an output element's contraction order does not depend on its row, and every other kernel of the loss works per clip or per element: here the
    two results must also be bitwise equal, which is what would catch one clip's data leaking into another's."""
    raw, rec, ref64, _ = _mel_refs("noise", "step", 3, 4100)
    batch = _run_mel(raw, rec)
    for b in range(3):
        one = _run_mel(raw[b:b + 1], rec[b:b + 1])
        same = all(torch.equal(o[0], t[b]) for o, t in zip(one, batch))
        for tag, got in (("alone", tuple(o[0] for o in one)), ("in the batch", tuple(t[b] for t in batch))):
            dev = (U.rel_err(got[0].reshape(1), ref64[0][b:b + 1]), U.rel_rms(got[1], ref64[1][b]), U.rel_rms(got[2], ref64[2][b]))
            print(f"[loss-edges] mel clip {b} of noise x step B=3 L=4100 {tag}: loss {dev[0]:.2e}   d_raw {dev[1]:.2e}   d_rec {dev[2]:.2e}   (bitwise equal: {same})")
            assert dev[0] <= LOSS_RTOL and dev[1] <= GRAD_TOL and dev[2] <= GRAD_TOL, (b, tag, dev)
        assert same, f"clip {b}: the B = 1 and the B = 3 result differ"


def test_mel_and_stft_loss_refusals():
    """The entry points check their own arguments: n_samples <= 1024 (the reflect padding of the 2048 window would read outside the clip), an empty batch, a sample rate
    below 2, null buffers.  Each returns ESCX_ERR_INVALID_ARG before anything is launched."""
    from esc import _native
    lib = _lib()
    x = torch.zeros(2, 2048, device="cuda"); loss = torch.zeros(2, device="cuda")
    bad = _native.ESCX_ERR_INVALID_ARG
    assert lib.escx_mel_loss_ex(_p(x), _p(x), 2, 1024, 16000, _p(loss), None, None, _stream()) == bad
    assert lib.escx_mel_loss_ex(_p(x), _p(x), 2, 0, 16000, _p(loss), None, None, _stream()) == bad
    assert lib.escx_mel_loss_ex(_p(x), _p(x), 0, 2048, 16000, _p(loss), None, None, _stream()) == bad
    assert lib.escx_mel_loss_ex(_p(x), _p(x), 2, 2048, 1, _p(loss), None, None, _stream()) == bad
    assert lib.escx_mel_loss_ex(None, _p(x), 2, 2048, 16000, _p(loss), None, None, _stream()) == bad
    assert lib.escx_mel_loss(_p(x), _p(x), 2, 1024, 16000, _p(loss), None, _stream()) == bad
    assert lib.escx_stft_loss_ex(_p(x), _p(x), 0, 2048, _p(loss), None, None, _stream()) == bad
    assert lib.escx_stft_loss_ex(_p(x), _p(x), 2, 0, _p(loss), None, None, _stream()) == bad
    assert lib.escx_stft_loss(_p(x), _p(x), 2, 2048, None, None, _stream()) == bad


# ---- GAN terms ----------------------------------------------------------------------------------------
SENTINEL = -12345.0
PAD_FILL = 1e30


def _gan_run(xb, refb, g, geo, B, mode, target, loss_init=None, accumulate=0, with_grad=True):
    """escx_gan_term (g is None) or escx_gan_term_grad on packed buffers; returns (loss or None, grad buffer or None) on the host."""
    lib = _lib()
    C, Cp, D0, D1, P1 = geo
    xd, rd = xb.cuda(), (None if refb is None else refb.cuda())
    grad = torch.full_like(xd, SENTINEL) if with_grad else None
    if g is None:
        loss = torch.full((B,), float("nan") if loss_init is None else loss_init, device="cuda")
        _check(lib.escx_gan_term(_p(xd), _p(rd), _p(grad), B, C, Cp, D0, D1, P1, mode, float(target), _p(loss), accumulate, _stream()))
    else:
        loss = None
        _check(lib.escx_gan_term_grad(_p(xd), _p(rd), _p(g.cuda()), _p(grad), B, C, Cp, D0, D1, P1, mode, float(target), _stream()))
    torch.cuda.synchronize()
    return (None if loss is None else loss.cpu()), (None if grad is None else grad.cpu())


def _gan_check_view(grad, geo):
    """Pad channels of the written view exactly 0, gap columns untouched, everything else finite."""
    C, Cp, D0, D1, P1 = geo
    assert bool((grad[:, :, :D1, C:] == 0).all()), "pad channels of the gradient view must be written as 0"
    assert bool((grad[:, :, D1:, :] == SENTINEL).all()), "the pitch-gap columns are not part of the view"
    assert bool(torch.isfinite(grad).all())


@pytest.mark.parametrize("geo,B", U.GAN_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gan_terms(geo, B):
    """escx_gan_term / escx_gan_term_grad on (C, Cp, D0, D1, P1) views: C < Cp (pad channels are loaded but must not count), P1 > D1 (a column slice of a wider buffer),
    more than 16384 float4 groups (second grid-stride trip), one element, 65 clips.  Pad channels and gap columns of x and ref hold 1e30, the gradient buffer a sentinel.
    Both modes, targets 0 and 1: loss within LOSS_RTOL and gradient within GRAD_TOL of float64; pad channels of the view written as exactly 0, gap columns still the sentinel;
    planted x == ref elements get exactly 0 in mode 1; accumulate = 1 adds to loss_dev and accumulate = 0 overwrites it; the per-clip upstream g scales clip b's gradient
    bitwise as a separate float32 multiply by g[b] * inv_n does."""
    C, Cp, D0, D1, P1 = geo
    x, ref, same = U.gan_case(geo, B)
    xb, refb = U.gan_pack(x, Cp, P1, PAD_FILL), U.gan_pack(ref, Cp, P1, PAD_FILL)
    gen = torch.Generator().manual_seed(B)
    g = torch.randn(B, generator=gen) * 3.0
    inv_n = np.float32(1.0) / (np.float32(C) * np.float32(D0) * np.float32(D1))
    for mode, target in ((0, 0.0), (0, 1.0), (1, 0.0)):
        tag = f"gan C={C} Cp={Cp} D0={D0} D1={D1} P1={P1} B={B} mode {mode} target {target:g}"
        l64, d64 = U.gan_reference(x, ref, mode, target)
        rb = refb if mode == 1 else None
        # forward with the unit gradient, loss_dev pre-set to NaN: accumulate = 0 overwrites
        loss, grad = _gan_run(xb, rb, None, geo, B, mode, target)
        _gan_check_view(grad, geo)
        e_loss, e_grad = U.rel_err(loss, l64), U.rel_rms(U.gan_unpack(grad, C, D1), d64)
        # the same without a gradient buffer, added to a pre-set loss_dev
        loss_acc, _ = _gan_run(xb, rb, None, geo, B, mode, target, loss_init=7.0, accumulate=1, with_grad=False)
        e_acc = U.rel_err(loss_acc, 7.0 + l64)
        assert torch.equal(loss_acc, (torch.full((B,), 7.0) + loss))
        # backward with the upstream gradient folded in
        _, gg = _gan_run(xb, rb, g, geo, B, mode, target)
        _gan_check_view(gg, geo)
        _, dg64 = U.gan_reference(x, ref, mode, target, g)
        got = U.gan_unpack(gg, C, D1)
        e_gg = U.rel_rms(got, dg64)
        print(f"[loss-edges] {tag}: loss {e_loss:.2e}   accumulated {e_acc:.2e}   grad {e_grad:.2e}   grad with upstream g {e_gg:.2e}")
        assert e_loss <= LOSS_RTOL and e_acc <= LOSS_RTOL and e_grad <= GRAD_TOL and e_gg <= GRAD_TOL
        gs = (g * torch.tensor(inv_n)).view(B, 1, 1, 1)             # float32, as the kernel forms it
        want = (-2.0 * (float(target) - x)) * gs if mode == 0 else torch.sign(x - ref) * gs
        assert torch.equal(got, want), f"{tag}: not the float32 product with g[b] * inv_n"
        if mode == 1:
            assert bool((U.gan_unpack(grad, C, D1)[same] == 0).all()) and bool((got[same] == 0).all())


def test_gan_term_error_paths():
    """mode 1 without ref, mode 2, a negative mode, B = 0, null x / loss / g / grad: ESCX_ERR_INVALID_ARG, nothing launched."""
    from esc import _native
    lib = _lib()
    bad = _native.ESCX_ERR_INVALID_ARG
    x = torch.zeros(2, 3, 3, 4, device="cuda"); loss = torch.zeros(2, device="cuda"); g = torch.ones(2, device="cuda"); grad = torch.zeros_like(x)
    a = (2, 3, 4, 3, 3, 3)              # B, C, Cp, D0, D1, P1
    assert lib.escx_gan_term(_p(x), None, None, *a, 1, 0.0, _p(loss), 0, _stream()) == bad
    assert lib.escx_gan_term(_p(x), _p(x), None, *a, 2, 0.0, _p(loss), 0, _stream()) == bad
    assert lib.escx_gan_term(_p(x), _p(x), None, *a, -1, 0.0, _p(loss), 0, _stream()) == bad
    assert lib.escx_gan_term(_p(x), None, None, 0, *a[1:], 0, 0.0, _p(loss), 0, _stream()) == bad
    assert lib.escx_gan_term(None, None, None, *a, 0, 0.0, _p(loss), 0, _stream()) == bad
    assert lib.escx_gan_term(_p(x), None, None, *a, 0, 0.0, None, 0, _stream()) == bad
    assert lib.escx_gan_term_grad(_p(x), None, _p(g), _p(grad), *a, 1, 0.0, _stream()) == bad
    assert lib.escx_gan_term_grad(_p(x), _p(x), _p(g), _p(grad), *a, 2, 0.0, _stream()) == bad
    assert lib.escx_gan_term_grad(_p(x), None, _p(g), _p(grad), 0, *a[1:], 0, 0.0, _stream()) == bad
    assert lib.escx_gan_term_grad(_p(x), None, None, _p(grad), *a, 0, 0.0, _stream()) == bad
    assert lib.escx_gan_term_grad(_p(x), None, _p(g), None, *a, 0, 0.0, _stream()) == bad
    assert lib.escx_gan_term(_p(x), None, None, *a, 0, 0.0, _p(loss), 0, _stream()) == 0          # and the good call goes through


# ---- flat optimiser -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 262144 + 257])
def test_flat_optimiser_sizes(n):
    """escx_grad_norm_clip + escx_adamw_step against a float64 restatement of clip_grad_norm_(0.5) + AdamW: one element, and n > 1024 x 256 where every thread of
    sumsq_partial_kernel takes a second grid-stride trip (with an odd tail).  Tolerances of tests/test_train.py::test_flat_adamw_and_clipping_match_torch."""
    lib = _lib()
    gen = torch.Generator().manual_seed(3 + n)
    p0 = torch.randn(n, generator=gen); grads = [torch.randn(n, generator=gen) * s for s in (0.01, 3.0, 0.2)]
    p = p0.clone().cuda(); m = torch.zeros(n, device="cuda"); v = torch.zeros(n, device="cuda")
    aux = torch.zeros(2 + 1024, device="cuda")
    for step, (gcpu, (norm, pref)) in enumerate(zip(grads, U.clip_adamw_reference(p0, grads, 0.5, 1e-3, 0.8, 0.95, 1e-8, 0.05)), 1):
        gg = gcpu.cuda()
        _check(lib.escx_grad_norm_clip(_p(gg), n, 0.5, _p(aux), _stream()))
        _check(lib.escx_adamw_step(_p(p), _p(gg), _p(m), _p(v), n, step, 1e-3, 0.8, 0.95, 1e-8, 0.05, _p(aux), _stream()))
        torch.cuda.synchronize()
        e_n = abs(float(aux[0]) - norm) / norm
        e_p = float(np.max(np.abs(p.cpu().numpy().astype(np.float64) - pref.numpy()) / (2e-5 * np.abs(pref.numpy()) + 2e-7)))
        print(f"[loss-edges] optimiser n={n} step {step}: norm {e_n:.2e}   parameters, worst error / tolerance {e_p:.2e}")
        assert e_n <= 1e-5
        np.testing.assert_allclose(p.cpu().numpy(), pref.numpy(), rtol=2e-5, atol=2e-7)
