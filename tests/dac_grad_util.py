"""Shared pieces of the decoder-gradient tests (tests/test_dac_grad.py, tests/test_dac_grad_host.py) and of tools/gen_dac_grad_golden.py:
the restatement of tests/dac_util.py in a chosen dtype, the latent gradient d_z = (d audio / d z)^T w by torch autograd on the CPU, and the
seeded inputs.  tests/golden/dac_grad.npz pins the float64 restatement to the REAL reference's DAC.decode under autograd."""
import json
import os

import numpy as np
import torch

import dac_util as du
from esc import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE_CASES = {"dac_syn": (3, 7), "dac_tiny": (2, 5)}          # name -> (batch, frames) of the cases stored in dac_grad.npz


class DacRefD(du.DacRef):
    """tests/dac_util.DacRef with the state_dict kept in `dtype` (DacRef itself casts to float32)."""

    def __init__(self, cfg, sd, dtype=torch.float64):
        super().__init__(cfg, sd)
        self.sd = {k: v.to(dtype) for k, v in sd.items()}


def config(name):
    return json.loads(str(np.load(os.path.join(GOLD, f"{name}.npz"))["config_json"]))


def manifest(name):
    with open(os.path.join(GOLD, f"{name}_manifest.json")) as f:
        return json.load(f)


def state_dict(name):
    return {k: torch.from_numpy(v) for k, v in synth.dac_state_dict(manifest(name)).items()}


def seeded(tag, shape, scale=1.0):
    """float64 array of float32-representable values in [-scale, scale), a pure function of (tag, shape)."""
    n = int(np.prod(shape))
    return (scale * synth.hashed_uniform("dac-grad:" + tag, n)).astype(np.float32).astype(np.float64).reshape(shape)


def inputs(name, B, T):
    """(z (B, D, T), w (B, 1, samples)) of one case, float64 arrays holding float32 values."""
    cfg = du.full_config(config(name))
    return seeded(f"z:{name}:{B}x{T}", (B, cfg["latent_dim"], T)), seeded(f"w:{name}:{B}x{T}", (B, 1, du.output_samples(cfg, T)))


def grad_of(decoder, z, w, dtype):
    """d_z of sum(decoder(z) * w) by autograd, as a float64 numpy array; z, w: numpy arrays."""
    zt = torch.from_numpy(np.array(z)).to(dtype).requires_grad_(True)
    audio = decoder(zt)
    (audio * torch.from_numpy(np.array(w)).to(dtype)).sum().backward()
    return zt.grad.double().numpy()


def oracle(name, z, w, dtype=torch.float64, sd=None):
    """The restatement's latent gradient on the CPU in `dtype`."""
    ref = DacRefD(config(name), state_dict(name) if sd is None else sd, dtype)
    return grad_of(ref.decoder, z, w, dtype)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300))
