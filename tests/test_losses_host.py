"""The conditions the GPU tests of the loss kernels (test_losses.py) rest on, checked on the host.

test_losses.py holds the kernels to the float64 reference at the project's absolute tolerances.  That is only a fair - and only a sharp - demand where the
loss is well conditioned at the chosen input: no mel cell near an L1 tie or near the clamp, and the reference's own float32 evaluation inside the same
tolerances.  These tests assert exactly that for every such case, so a changed seed, shape or gain that breaks it fails HERE, on any machine, and cannot
quietly turn a GPU test into one that proves nothing.  If a case fails, change its input, not the bound.
"""
import numpy as np
import pytest
import torch

import loss_util as U


def _mel_conditions(raw, rec, tag, sample_rate=U.SR, weights=None):
    lin, log, clamp = U.tie_margins(raw, rec, sample_rate)
    l64, a64, b64 = U.mel_reference(raw, rec, torch.float64, sample_rate, weights)
    l32, a32, b32 = U.mel_reference(raw, rec, torch.float32, sample_rate, weights)
    el, ea, eb = U.rel_err(l32, l64), U.rel_rms(a32, a64), U.rel_rms(b32, b64)
    print(f"[loss-host mel {tag}] margins lin {lin:.2e} log {log:.2e} clamp {clamp:.2e}   float32 oracle: loss {el:.2e}  d_raw {ea:.2e}  d_rec {eb:.2e}")
    assert min(lin, log, clamp) >= U.TIE_MARGIN, f"{tag}: tie margins {lin:.2e} / {log:.2e} / {clamp:.2e}"
    assert el <= U.LOSS_RTOL, f"{tag}: float32 oracle loss {el:.2e} from float64"
    assert ea <= U.GRAD_TOL and eb <= U.GRAD_TOL, f"{tag}: float32 oracle gradients {ea:.2e} / {eb:.2e} from float64"


@pytest.mark.parametrize("L", U.MEL_LENGTHS)
def test_well_conditioned_mel_cases_are_well_conditioned(L):
    """Every (clip, gain, B) of test_losses.py's well-conditioned mel cases at this length: tie margins >= 1e-5 in all three measures and the float32
    oracle within LOSS_RTOL / GRAD_TOL of float64 (value, both gradients)."""
    for kind, gain, B, Lc in U.MEL_WELL:
        if Lc == L:
            _mel_conditions(*U.mel_case(kind, gain, B, L), f"{kind} x {gain} B={B} L={L}")


def test_the_other_bounded_mel_cases_are_well_conditioned():
    """The B = 65 case, the below-clamp clip (only the linear term survives), the module case with unequal weights, the 8 kHz case, the two
    silent-against-noise cases, and one clip of the scratch-reuse and batch-independence tests."""
    kind, gain, B, L = U.MEL_WELL_B65
    _mel_conditions(*U.mel_case(kind, gain, B, L, U.MEL_WELL_B65_SEED), f"{kind} x {gain} B={B} L={L}")
    kind, gain, B, L = U.MEL_BELOW_CLAMP
    raw, rec = U.mel_case(kind, gain, B, L)
    _mel_conditions(raw, rec, f"{kind} x {gain} B={B} L={L}")
    for w, nm in zip(U.O.MEL_WINDOWS, U.O.MEL_BINS):            # ... and it IS below the clamp everywhere, on both sides
        assert float(U.O.mel_spectrogram(raw.double(), w, nm).max()) < U.CLAMP_EPS
    kind, gain, B, L = U.MEL_MODULE
    _mel_conditions(*U.mel_case(kind, gain, B, L), f"module {kind} x {gain} B={B} L={L}", weights=U.MEL_MODULE_WEIGHTS)
    kind, gain, B, L = U.MEL_RATE
    _mel_conditions(*U.mel_case(kind, gain, B, L), f"8 kHz {kind} x {gain} B={B} L={L}", sample_rate=8000)
    noise = U.noise_clip(2, 2049, 41)
    _mel_conditions(U.silent_clip(2, 2049), noise, "silent raw, noise recon")
    _mel_conditions(noise, U.silent_clip(2, 2049), "noise raw, silent recon")
    _mel_conditions(*U.mel_case("noise", "step", 3, 6000), "noise x step B=3 L=6000")


def test_at_clamp_cases_straddle_the_clamp():
    """The at_clamp clip has mel cells with exactly one side below clamp_eps - the recon side at gain 0.5, the raw side at 1.7: the cells where the `>= clamp_eps` branches of
    mel_l1_kernel decide the gradient (with both sides below, the log term is 0 whatever the branch does; with a silent side, |S| = 0 kills the gradient anyway)."""
    n_rec, _ = U.clamp_straddles(*U.mel_case("at_clamp", "half", 2, 2049))
    _, n_raw = U.clamp_straddles(*U.mel_case("at_clamp", "up", 2, 2049))
    print(f"[loss-host at_clamp] cells with only the recon side clamped (x 0.5): {n_rec}   only the raw side clamped (x 1.7): {n_raw}")
    assert min(n_rec, n_raw) >= U.MEL_AT_CLAMP_MIN_CELLS
    assert ("at_clamp", "half", 2, 2049) in U.MEL_WELL and ("at_clamp", "up", 2, 2049) in U.MEL_WELL


def test_raw_plus_noise_would_not_do():
    """The input the older tests use (rec = raw + independent noise, here at their (3, 6000)) violates the conditions: a cell 1e-8 from a tie, and the float32 oracle's own
    gradient 6e-4 from float64.  The reason for the scaled reconstructions, and the proof that the check above can fail."""
    raw = U.noise_clip(3, 6000, 5)
    rec = raw + 0.03 * U.noise_clip(3, 6000, 6, amp=1.0)
    lin, log, _ = U.tie_margins(raw, rec)
    assert min(lin, log) < U.TIE_MARGIN
    _, _, b64 = U.mel_reference(raw, rec, torch.float64)
    _, _, b32 = U.mel_reference(raw, rec, torch.float32)
    assert U.rel_rms(b32, b64) > U.GRAD_TOL
    with pytest.raises(AssertionError):
        _mel_conditions(raw, rec, "raw + noise B=3 L=6000")


def test_harmonic_clip_is_what_it_says():
    """Loss value well conditioned (float32 oracle within LOSS_RTOL), no ties, and near-empty bins: the smallest mel value is orders below the largest."""
    for kind, gain, B, L in U.MEL_HARMONIC:
        raw, rec = U.mel_case(kind, gain, B, L)
        lin, log, clamp = U.tie_margins(raw, rec)
        l64, a64, b64 = U.mel_reference(raw, rec, torch.float64)
        l32, a32, b32 = U.mel_reference(raw, rec, torch.float32)
        print(f"[loss-host harmonic x {gain} B={B} L={L}] margins {lin:.2e} {log:.2e} {clamp:.2e}   float32 oracle: loss {U.rel_err(l32, l64):.2e}  "
              f"d_raw {U.rel_rms(a32, a64):.2e}  d_rec {U.rel_rms(b32, b64):.2e}")
        assert min(lin, log) >= U.TIE_MARGIN
        assert U.rel_err(l32, l64) <= U.LOSS_RTOL
    m = U.O.mel_spectrogram(raw.double(), 2048, 320)
    assert float(m.min()) < 1e-3 * float(m.max())


@pytest.mark.parametrize("B,per_clip", U.STFT_CASES)
def test_stft_cases_are_well_conditioned(B, per_clip):
    """float32 oracle within LOSS_RTOL / GRAD_TOL of float64 on the planted inputs - over everything and, so that the few huge gradients at +-1e-12 cannot
    hide the rest, over the unplanted elements alone; and the plants are where the GPU test expects them."""
    raw, rec, planted = U.stft_case(B, per_clip)
    l64, a64, b64 = U.stft_reference(raw, rec, torch.float64)
    l32, a32, b32 = U.stft_reference(raw, rec, torch.float32)
    assert U.rel_err(l32, l64) <= U.LOSS_RTOL
    assert U.rel_rms(a32, a64) <= U.GRAD_TOL and U.rel_rms(b32, b64) <= U.GRAD_TOL
    keep = ~planted.numpy()
    if keep.any():
        assert U.rel_rms(a32[keep], a64[keep]) <= U.GRAD_TOL and U.rel_rms(b32[keep], b64[keep]) <= U.GRAD_TOL
    assert (rec == 0).any() and np.all(b64[(rec == 0).numpy()] == 0.0)          # float64: exactly zero gradient at an exact zero
    if per_clip > 1:
        assert (raw == 0).any() and ((raw == 0) & (rec == 0)).any() and np.all(a64[(raw == 0).numpy()] == 0.0)
        assert (rec.abs() == 1e-12).any() and (raw.abs() == 1e-12).any() and (rec == 3e3).any() and (raw == -3e3).any()
    if per_clip > 16384:
        assert planted[:, 16384:].any()


def test_gan_pack_round_trip_and_reference():
    """gan_unpack(gan_pack(x)) == x with the fill in every pad channel and gap column; the float64 reference against autograd."""
    for (C, Cp, D0, D1, P1), B in U.GAN_CASES:
        x, ref, same = U.gan_case((C, Cp, D0, D1, P1), B)
        buf = U.gan_pack(x, Cp, P1, fill=1e30)
        assert buf.shape == (B, D0, P1, Cp)
        assert torch.equal(U.gan_unpack(buf, C, D1), x)
        assert bool((buf[:, :, :, C:] == 1e30).all()) and bool((buf[:, :, D1:, :] == 1e30).all())
        assert int((buf != 1e30).sum()) == x.numel()
        assert bool(same.view(B, -1).any(1).all()) and torch.equal(ref[same], x[same]) and bool((ref[~same] != x[~same]).all())
    x, ref, _ = U.gan_case(U.GAN_GEOMETRIES[1], 3)
    g = torch.tensor([0.5, -2.0, 3.0], dtype=torch.float64)
    for mode, target in ((0, 0.0), (0, 1.0), (1, 0.0)):
        xa = x.double().requires_grad_(True)
        loss = ((target - xa) ** 2).mean([1, 2, 3]) if mode == 0 else (xa - ref.double()).abs().mean([1, 2, 3])
        (loss * g).sum().backward()
        l, d = U.gan_reference(x, ref, mode, target, g)
        np.testing.assert_allclose(l, loss.detach().numpy(), rtol=1e-14)
        np.testing.assert_allclose(d, xa.grad.numpy(), rtol=1e-14, atol=0)


def test_clip_adamw_restatement_against_torch():
    """The float64 restatement the GPU test uses == clip_grad_norm_ + torch.optim.AdamW in float64."""
    gen = torch.Generator().manual_seed(3)
    p0 = torch.randn(1000, generator=gen, dtype=torch.float64)
    grads = [torch.randn(1000, generator=gen, dtype=torch.float64) * s for s in (0.01, 3.0, 0.2)]
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([ref], lr=1e-3, betas=(0.8, 0.95), eps=1e-8, weight_decay=0.05)
    for g, (norm, p) in zip(grads, U.clip_adamw_reference(p0, grads, 0.5, 1e-3, 0.8, 0.95, 1e-8, 0.05)):
        ref.grad = g.clone()
        tn = torch.nn.utils.clip_grad_norm_([ref], 0.5)
        opt.step()
        assert abs(norm - float(tn)) <= 1e-12 * norm
        np.testing.assert_allclose(p.numpy(), ref.detach().numpy(), rtol=1e-12, atol=1e-15)
