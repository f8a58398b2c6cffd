"""Shared pieces of the stand-alone quantiser's tests (tests/test_dac_quantizer.py, tests/test_dac_quantizer_host.py) and of
tools/gen_dac_quantizer_golden.py: the fixture's cases and seeded cotangents, models built from a configuration with name-keyed weights, and the
gradients of sum(z_q * w_z) + sum(latents * w_lat) + cm * w_cm (+ cb * w_cb) of `quantizer(z)` with respect to z and to every quantiser parameter
by torch autograd of the restatement of tests/dac_encode_grad_util.py (DacRefE.quantize) on the CPU in a chosen dtype.
tests/golden/dac_quantizer.npz pins the float64 restatement to the REAL reference's ResidualVectorQuantize under autograd.

Fixture layout, (B, T, n) = CASES[name]; float32 unless said otherwise:
    {name}_seed                          the clip seed the generator settled on (every stored margin is at least MIN_MARGIN)
    {name}_z                             the reference encoder's output (B, D, T)
    {name}_zq_{nkey}, _codes_{nkey} (int16), _cm_{nkey}, _cb_{nkey}      reference quantizer(z, n) for n in dac_util.GOLDEN_NS (z_q once per distinct n)
    {name}_latents, {name}_margins       latents at every codebook (a smaller n is their prefix); second-best minus best distance (B, n, T)
    {name}_counts (int64), _zq_clip, _cm_clip, _cb_clip                   one per-clip count vector (the reference's training-mode mask, quantize.py:181-190)
    {name}_fl_zq, _fl_zp, _fl_codes (int16)                               from_latents on the full latents
    {name}_flr_zq, _flr_codes (int16), _flr_channels (int64)              from_latents on a slice with a non-zero channel remainder
    {name}_d_z, {name}_d_z_clip (dac_syn) (float64)                       reference float64 autograd for the seeded cotangents
    dac_syn_g/{key} (float64)                                             every quantiser parameter's gradient, the codebook loss' cotangent included
"""
import numpy as np
import torch

import dac_encode_grad_util as eu
import dac_encode_param_grad_util as pu
from esc import synth

du = eu.du
CASES = {"dac_syn": (3, 7, 4), "dac_tiny": (2, 5, 18), "dac_base": (1, 3, 18)}       # name -> (clips, frames, codebooks)
MIN_MARGIN = 1e-5                                                                  # the floor tools/gen_dac_chunk_golden.py states for its fixtures
VARIANTS = {"J2": dict(latent_dim=96), "J4": dict(latent_dim=192), "K100": dict(codebook_size=100)}      # of dac_syn: the kernels' other paths


def hop(name):
    return int(np.prod(eu.config(name)["encoder_rates"]))


def clips(name, seed):
    """(B, 1, T * hop) float32 audio of the case: a noise clip, then voiced clips, name- and seed-keyed."""
    B, T, _ = CASES[name]
    L = T * hop(name)
    pcm = [synth.noise_clip_int16(f"dacq-noise-{name}-{seed}", L)] + [synth.voiced_clip_int16(f"dacq-voiced-{name}-{seed}-{b}", L) for b in range(1, B)]
    return torch.from_numpy(synth.pcm_to_float(np.stack(pcm)))[:, None]


def cotangents(name, per_clip=False):
    """{"z", "latents", "cm", "cb"}: float64 arrays holding float32 values, a pure function of the case.  The losses are means over B d T
    elements, so their cotangents are seeded values in [0.5, 1) times d T (dac_encode_grad_util.inputs' scheme)."""
    B, T, n = CASES[name]
    cfg = du.full_config(eu.config(name))
    D, d = cfg["latent_dim"], cfg["codebook_dim"]
    tag = f"quantizer:{name}:{B}x{T}:n{n}" + (":clip" if per_clip else "")
    scal = lambda k: np.float64(np.float32((0.75 + 0.25 * float(eu.seeded(k + tag, (1,))[0])) * d * T))       # noqa: E731
    return {"z": eu.seeded("w_zq:" + tag, (B, D, T)), "latents": eu.seeded("w_lat:" + tag, (B, n * d, T)), "cm": scal("w_cm:"), "cb": scal("w_cb:")}


def quantizer_keys(sd):
    return [k for k in sd if k.startswith("quantizer.")]


def variant(which):
    """(config, state_dict) of dac_syn with one changed keyword and name-keyed weights over the model's own manifest."""
    from esc.baselines import DAC
    cfg = dict(eu.config("dac_syn"), **VARIANTS[which])
    man = {k: list(v.shape) for k, v in DAC(**cfg).state_dict().items()}
    return cfg, {k: torch.from_numpy(v) for k, v in synth.dac_state_dict(man).items()}


def model_of(cfg, sd, device="cuda"):
    from esc.baselines import DAC
    m = DAC(**cfg)
    m.load_state_dict(sd, strict=True)
    return m.to(device).eval()


def _t(a, dtype=np.int64):
    return None if a is None else torch.from_numpy(np.array(a, dtype))


def run_ref(cfg, sd, z, n=None, dtype=torch.float64, codes=None, counts=None):
    """DacRefE.quantize on z (numpy) in `dtype` without gradients: {"z", "codes", "latents", "cm", "cb"} as numpy (float64 / int64)."""
    ref = eu.DacRefE(cfg, sd, dtype)
    with torch.no_grad():
        zq, c, lat, cm, cb, _ = ref.quantize(torch.from_numpy(np.array(z)).to(dtype), n, codes=_t(codes), counts=_t(counts))
    return {"z": zq.double().numpy(), "codes": c.numpy(), "latents": lat.double().numpy(), "cm": float(cm), "cb": float(cb)}


def grads(cfg, sd, z, cot, n=None, dtype=torch.float64, codes=None, counts=None, params=False):
    """(d_z, {key: gradient or None}) of sum_k sum(out[k] * cot[k]) of the restatement's quantiser by autograd on the CPU in `dtype`, float64
    numpy arrays; with params the quantiser's parameters are leaves too (a stage the call does not run has None)."""
    ref = eu.DacRefE(cfg, sd, dtype)
    leaves = {}
    if params:
        for k in quantizer_keys(ref.sd):
            ref.sd[k] = ref.sd[k].detach().clone().requires_grad_(True)
            leaves[k] = ref.sd[k]
    zt = torch.from_numpy(np.array(z)).to(dtype).requires_grad_(True)
    zq, _, lat, cm, cb, _ = ref.quantize(zt, n, codes=_t(codes), counts=_t(counts))
    out = {"z": zq, "latents": lat, "cm": cm, "cb": cb}
    sum((out[k] * torch.from_numpy(np.asarray(w, np.float64)).to(dtype)).sum() for k, w in cot.items()).backward()
    return zt.grad.double().numpy(), {k: None if p.grad is None else p.grad.double().numpy() for k, p in leaves.items()}


def device_grads(model, z, cot, n, keys=()):
    """(outputs, z.grad, {key: p.grad or None}) of the same loss through model.quantizer on the device; z, cot: numpy."""
    dev = next(model.parameters()).device
    for p in model.parameters():
        p.grad = None
    zt = torch.from_numpy(np.asarray(z, np.float32)).to(dev).requires_grad_(True)
    out = model.quantizer(zt, n)
    named = dict(zip(("z", "codes", "latents", "cm", "cb"), out))
    loss = sum((named[k] * torch.from_numpy(np.asarray(w, np.float32)).to(dev)).sum() for k, w in cot.items())
    loss.backward()
    ps = dict(model.named_parameters())
    return out, zt.grad, {k: None if ps[k].grad is None else ps[k].grad.detach().double().cpu().numpy() for k in keys}
