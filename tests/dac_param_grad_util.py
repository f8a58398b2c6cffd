"""Shared pieces of the decoder parameter-gradient tests (tests/test_dac_param_grad.py, tests/test_dac_param_grad_host.py) and of
tools/gen_dac_param_grad_golden.py: the gradient of sum(decode(z) * w) with respect to every decoder parameter by torch autograd of the
restatement of tests/dac_util.py on the CPU in a chosen dtype, the fixture's layout, and the error rule.
tests/golden/dac_param_grad.npz pins the float64 restatement to the REAL reference's DAC.decode under autograd.

Fixture layout (float64 throughout):
    {name}_z, {name}_w                  the seeded inputs of dac_grad_util.inputs(name, B, T), (B, T) = FIXTURE_CASES[name]
    {name}_g/{key}                      the full gradient of decoder parameter `key`                 (dac_syn: every key; dac_tiny: bias, weight_g, alpha)
    {name}_n/{key}, {name}_s/{key}      its norm and its values at sample_index(key, numel)         (dac_tiny's weight_v: 2.49 M weights in all)
"""
import numpy as np
import torch

import dac_grad_util as gu
from esc import synth

FIXTURE_CASES = {"dac_syn": (3, 7), "dac_tiny": (2, 5)}
SAMPLED = {"dac_tiny": ("weight_v",)}                             # kinds stored as norm + samples
KINDS = ("bias", "weight_g", "weight_v", "alpha")
MAX_SAMPLES = 256


def kind(key):
    return key.rsplit(".", 1)[1]


def decoder_keys(sd):
    return [k for k in sd if k.startswith("decoder.")]


def sample_index(key, numel):
    """At most MAX_SAMPLES distinct flat positions of a tensor of numel values, a pure function of (key, numel); every position when it is small."""
    if numel <= MAX_SAMPLES:
        return np.arange(numel)
    u = synth.hashed_uniform("dac-param-grad:idx:" + key, 4 * MAX_SAMPLES)          # in [-1, 1)
    idx = np.unique(np.minimum(((u + 1.0) * 0.5 * numel).astype(np.int64), numel - 1))
    return idx[:MAX_SAMPLES]


def grads_of(decode, params, z, w, dtype, mse=False):
    """{key: float64 gradient of sum(decode(z) * w), or with mse of mean((decode(z) - w)^2)} for the leaf tensors `params` ({key: tensor that
    requires grad}); z, w: numpy arrays."""
    audio = decode(torch.from_numpy(np.array(z)).to(dtype))
    wt = torch.from_numpy(np.array(w)).to(dtype)
    ((audio - wt).pow(2).mean() if mse else (audio * wt).sum()).backward()
    return {k: p.grad.double().numpy() for k, p in params.items()}


def oracle(name, z, w, dtype=torch.float64, sd=None, mse=False):
    """The restatement's decoder parameter gradients on the CPU in `dtype`, keyed in state_dict order."""
    ref = gu.DacRefD(gu.config(name), gu.state_dict(name) if sd is None else sd, dtype)
    params = {}
    for k in decoder_keys(ref.sd):
        ref.sd[k] = ref.sd[k].detach().clone().requires_grad_(True)
        params[k] = ref.sd[k]
    return grads_of(ref.decoder, params, z, w, dtype, mse)


def errors(got, want):
    """{key: |g - g_f64| / |g_f64|} over the keys of `want`."""
    return {k: gu.rel_l2(got[k], want[k]) for k in want}


def by_kind(err):
    """{kind: (rms over the kind's tensors, largest, key of the largest)}"""
    out = {}
    for kd in KINDS:
        e = {k: v for k, v in err.items() if kind(k) == kd}
        worst = max(e, key=e.get)
        out[kd] = (float(np.sqrt(np.mean(np.square(list(e.values()))))), e[worst], worst)
    return out


def check_rule(err_dev, err_eager, label, factor=2.0):
    """The project's rule per kind: rms(err_dev) <= 2 rms(err_eager), and every tensor's err_dev <= 2 max(err_eager) of its kind.  Prints every
    figure before it asserts."""
    dev, eag = by_kind(err_dev), by_kind(err_eager)
    for kd in KINDS:
        print(f"{label} {kd:9s}: rms dev {dev[kd][0]:.3e} eager {eag[kd][0]:.3e} ratio {dev[kd][0] / eag[kd][0]:.2f} | "
              f"max dev {dev[kd][1]:.3e} ({dev[kd][2]}) eager {eag[kd][1]:.3e} ratio {dev[kd][1] / eag[kd][1]:.2f}")
    for kd in KINDS:
        assert 1e-9 < eag[kd][0] < 1e-4, (kd, eag[kd])           # the yardstick itself is float32 arithmetic, not something broken
        assert dev[kd][0] <= factor * eag[kd][0], (label, kd, "rms", dev[kd][0], eag[kd][0])
        assert dev[kd][1] <= factor * eag[kd][1], (label, kd, "max", dev[kd][2], dev[kd][1], eag[kd][1])
