"""Shared pieces of the encoder / quantiser parameter-gradient tests (tests/test_dac_encode_param_grad.py,
tests/test_dac_encode_param_grad_host.py) and of tools/gen_dac_encode_param_grad_golden.py: the gradient of
sum(z * w_z) + sum(latents * w_lat) + cm * w_cm + cb * w_cb of encode (or of sum(audio * w_audio) of the eval forward) with respect to every
parameter by torch autograd of the restatement of tests/dac_encode_grad_util.py (DacRefE, the parameters as leaves) on the CPU in a chosen dtype,
the fixture's layout, and the error rule.  tests/golden/dac_encode_param_grad.npz pins the float64 restatement to the REAL reference's DAC.encode
under autograd.

Fixture layout (float64 unless said otherwise), (B, L, n) = dac_encode_grad_util.FIXTURE_CASES[name].  The audio x and the cotangents on z, latents
and the commitment loss are dac_encode_grad.npz's, seeded by inputs(name, B, L, n), and are not stored again:
    {name}_w_cb                         the seeded cotangent on the codebook loss
    {name}_codes                        the codes the reference chose (int16)
    {name}_g/{key}                      the full gradient of parameter `key`                        (dac_syn: every key; dac_tiny: bias, weight_g, alpha)
    {name}_s/{key}                      its values at sample_index(key, numel)                      (dac_tiny's weight_v and codebook.weight)
    {name}_norms                        the norms of the sampled tensors, in sampled_keys order     (one array: a zip member per scalar costs more than the scalar)
"""
import numpy as np
import torch

import dac_encode_grad_util as eu
import dac_param_grad_util as pu
from esc import synth

gu = eu.gu
FIXTURE_CASES = eu.FIXTURE_CASES
SAMPLED = {"dac_tiny": ("weight_v", "codebook")}                  # kinds stored as norm + samples
KINDS = ("bias", "weight_g", "weight_v", "alpha", "codebook")
U32 = 2.0 ** -24                                                  # unit round-off of the fp32 storage: no eager error counts as lower
MAX_SAMPLES = 48                                                 # per sampled tensor: 84 sampled tensors keep the fixture under the largest DAC fixture


def kind(key):
    return "codebook" if key.endswith("codebook.weight") else key.rsplit(".", 1)[1]


def sample_index(key, numel):
    """At most MAX_SAMPLES distinct flat positions spread over a tensor of numel values, a pure function of (key, numel); every position when
    it is small (dac_param_grad_util.sample_index's scheme with a smaller budget and no truncation of the sorted draw)."""
    if numel <= MAX_SAMPLES:
        return np.arange(numel)
    u = synth.hashed_uniform("dac-encode-param-grad:idx:" + key, MAX_SAMPLES)       # in [-1, 1)
    return np.unique(np.minimum(((u + 1.0) * 0.5 * numel).astype(np.int64), numel - 1))


def sampled_keys(name, keys):
    """The keys of `keys` the fixture stores as norm + samples, in order."""
    return [k for k in keys if kind(k) in SAMPLED.get(name, ())]


def encode_keys(sd):
    """The encoder's and the quantiser's keys in state_dict order."""
    return [k for k in sd if k.startswith(("encoder.", "quantizer."))]


def stage_of(key):
    """The quantiser stage of a `quantizer.quantizers.{i}.*` key, else None."""
    return int(key.split(".")[2]) if key.startswith("quantizer.quantizers.") else None


def inputs(name, B, L, n=None):
    """dac_encode_grad_util.inputs plus the cotangent "cb" on the codebook loss: like the commitment loss it is a mean over B d T elements, so
    its cotangent is a seeded value in [0.5, 1) times d T."""
    x, cot = eu.inputs(name, B, L, n)
    _, T, n, d = eu.shapes(name, B, L, n)
    cot = dict(cot)
    cot["cb"] = np.float64(np.float32((0.75 + 0.25 * float(eu.seeded(f"w_cb:{name}:{B}x{L}:n{n}", (1,))[0])) * d * T))
    return x, cot


def grads_of(fn, params, x, cotangents, dtype):
    """{key: float64 gradient, or None for a leaf that is not on the graph} of sum_k sum(fn(x)[k] * cotangents[k])."""
    out = fn(torch.from_numpy(np.array(x)).to(dtype))
    loss = sum((out[k] * torch.from_numpy(np.asarray(w, np.float64)).to(dtype)).sum() for k, w in cotangents.items())
    loss.backward()
    return {k: None if p.grad is None else p.grad.double().numpy() for k, p in params.items()}


def oracle(name, x, cotangents, n=None, dtype=torch.float64, codes=None, counts=None, whole=False, sd=None):
    """The restatement's parameter gradients on the CPU in `dtype`, keyed in state_dict order: the encoder's and the quantiser's for encode's
    outputs, or with whole=True every parameter's for the eval forward's (the cotangent key "audio" then exists too).  A quantiser stage the
    call does not run has None."""
    ref = eu.DacRefE(eu.config(name), eu.state_dict(name) if sd is None else sd, dtype)
    params = {}
    for k in (list(ref.sd) if whole else encode_keys(ref.sd)):
        ref.sd[k] = ref.sd[k].detach().clone().requires_grad_(True)
        params[k] = ref.sd[k]
    fn = ref.forward_dict if whole else ref.encode_dict
    return grads_of(lambda xt: fn(xt, n, eu._t(codes), eu._t(counts)), params, x, cotangents, dtype)


def with_fixture(name, g64, fixture):
    """g64 with every tensor the fixture stores in full taken from it."""
    out = dict(g64)
    for k in g64:
        if f"{name}_g/{k}" in fixture.files:
            out[k] = fixture[f"{name}_g/{k}"]
    return out


def errors(got, want):
    """{key: |g - g_f64| / |g_f64|} over the keys of `want` that have a gradient."""
    return {k: gu.rel_l2(got[k], w) for k, w in want.items() if w is not None}


def by_kind(err):
    """{kind: (rms over the kind's tensors, largest, key of the largest)}"""
    out = {}
    for kd in KINDS:
        e = {k: v for k, v in err.items() if kind(k) == kd}
        if e:
            worst = max(e, key=e.get)
            out[kd] = (float(np.sqrt(np.mean(np.square(list(e.values()))))), e[worst], worst)
    return out


def check_rule(err_dev, err_eager, label, factor=2.0):
    """dac_param_grad_util.check_rule with the fifth kind and the floor: per kind rms(err_dev) <= 2 rms(err_eager), and every tensor's err_dev <=
    2 max(err_eager) of its kind, each eager error taken no lower than 2^-24.  Prints every figure before it asserts."""
    eag_f = {k: max(v, U32) for k, v in err_eager.items()}
    dev, eag = by_kind(err_dev), by_kind(eag_f)
    assert set(dev) == set(eag), (label, sorted(dev), sorted(eag))
    for kd in dev:
        print(f"{label} {kd:9s}: rms dev {dev[kd][0]:.3e} eager {eag[kd][0]:.3e} ratio {dev[kd][0] / eag[kd][0]:.2f} | "
              f"max dev {dev[kd][1]:.3e} ({dev[kd][2]}) eager {eag[kd][1]:.3e} ratio {dev[kd][1] / eag[kd][1]:.2f}")
    for kd in dev:
        assert eag[kd][0] < 1e-4, (kd, eag[kd])                  # the yardstick itself is float32 arithmetic, not something broken
        assert dev[kd][0] <= factor * eag[kd][0], (label, kd, "rms", dev[kd][0], eag[kd][0])
        assert dev[kd][1] <= factor * eag[kd][1], (label, kd, "max", dev[kd][2], dev[kd][1], eag[kd][1])
