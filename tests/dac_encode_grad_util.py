"""Shared pieces of the encoder-gradient tests (tests/test_dac_encode_grad.py, tests/test_dac_encode_grad_host.py) and of
tools/gen_dac_encode_grad_golden.py: the restatement of tests/dac_util.py with the reference quantiser's detaches (nn/quantize.py:61-66; DacRef's
own `quantize` has none, so its autograd is not the reference's), the audio gradient by torch autograd on the CPU in a chosen dtype, and the
seeded inputs.  tests/golden/dac_encode_grad.npz pins the float64 restatement to the REAL reference's DAC.encode under autograd."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import dac_grad_util as gu

du = gu.du
config, state_dict, seeded, rel_l2, GOLD = gu.config, gu.state_dict, gu.seeded, gu.rel_l2, gu.GOLD
FIXTURE_CASES = {"dac_syn": (3, 28, 4), "dac_tiny": (2, 1600, 18)}          # name -> (batch, samples, n_quantizers) of the cases in dac_encode_grad.npz


class DacRefE(gu.DacRefD):
    """DacRefD whose quantiser is the reference's under autograd: the commitment loss sees the codebook vector detached, the codebook loss the
    latent detached, and the straight-through estimator passes the cotangent of z_q to z_e (quantize.py:58-70).  `codes` (B, n, T) forces every
    choice (entries below 0, the per-clip form's empty slots, are read as 0 and masked); `counts` (B,) runs clip b for counts[b] stages the way
    the library's per-clip encode does: z_q, the latents and the loss terms of the later stages are masked out (quantize.py:181-190)."""

    def quantize(self, z, n=None, force=None, margins=False, codes=None, counts=None):
        assert not force and not margins, "forced positions and margins are tests/dac_util.DacRef's"
        nc = self.cfg["n_codebooks"]
        n = nc if n is None else min(n, nc)
        zq, residual, cm, cb = 0, z, 0, 0
        out_codes, lats = [], []
        for i in range(n):
            p = f"quantizer.quantizers.{i}."
            ze = self._conv(residual, p + "in_proj.")
            idx = self._codebook_search(i, ze.detach())[1] if codes is None else codes[:, i].clamp_min(0)
            q = F.embedding(idx, self.sd[p + "codebook.weight"]).transpose(1, 2)
            cm_i = F.mse_loss(ze, q.detach(), reduction="none").mean([1, 2])
            cb_i = F.mse_loss(q, ze.detach(), reduction="none").mean([1, 2])
            q = self._conv(ze + (q - ze).detach(), p + "out_proj.")
            if counts is not None:
                mask = (i < counts).to(z.dtype)
                q_used, cm_i, cb_i, ze_out = q * mask[:, None, None], cm_i * mask, cb_i * mask, ze * mask[:, None, None]
            else:
                q_used, ze_out = q, ze
            zq = zq + q_used
            residual = residual - q
            cm = cm + cm_i.mean()
            cb = cb + cb_i.mean()
            out_codes.append(idx)
            lats.append(ze_out)
        return zq, torch.stack(out_codes, 1), torch.cat(lats, 1), cm, cb, None

    def encode_dict(self, x, n=None, codes=None, counts=None):
        z, c, lat, cm, cb, _ = self.quantize(self.encoder(x), n, codes=codes, counts=counts)
        return {"z": z, "codes": c, "latents": lat, "cm": cm, "cb": cb}

    def forward_dict(self, x, n=None, codes=None, counts=None):
        L = x.shape[-1]
        out = self.encode_dict(F.pad(x, (0, math.ceil(L / self.hop) * self.hop - L)), n, codes, counts)
        out["audio"] = self.decoder(out["z"])[..., :L]
        return out


def shapes(name, B, L, n=None):
    """(latent_dim, frames, stages, codebook_dim) of one case."""
    cfg = du.full_config(config(name))
    n = cfg["n_codebooks"] if n is None else min(n, cfg["n_codebooks"])
    return cfg["latent_dim"], du.num_frames(cfg, L), n, cfg["codebook_dim"]


def inputs(name, B, L, n=None):
    """(x (B, 1, L), {"z": w_z, "latents": w_lat, "cm": w_cm}) of one case: float64 arrays holding float32 values.  The commitment loss is a mean
    over B d T elements, so its cotangent is a seeded value in [0.5, 1) times d T: the term then weighs in x.grad like the other two."""
    D, T, n, d = shapes(name, B, L, n)
    tag = f"{name}:{B}x{L}:n{n}"
    w_cm = np.float64(np.float32((0.75 + 0.25 * float(seeded("w_cm:" + tag, (1,))[0])) * d * T))
    return seeded("x:" + tag, (B, 1, L), 0.5), {"z": seeded("w_z:" + tag, (B, D, T)), "latents": seeded("w_lat:" + tag, (B, n * d, T)), "cm": w_cm}


def grad_of(fn, x, cotangents, dtype):
    """d_x of sum_k sum(fn(x)[k] * cotangents[k]) by autograd, as a float64 numpy array; x and the cotangents are numpy arrays or scalars."""
    xt = torch.from_numpy(np.array(x)).to(dtype).requires_grad_(True)
    out = fn(xt)
    loss = sum((out[k] * torch.from_numpy(np.asarray(w, np.float64)).to(dtype)).sum() for k, w in cotangents.items())
    loss.backward()
    return xt.grad.double().numpy()


def _t(a):
    return None if a is None else torch.from_numpy(np.array(a, np.int64))


def oracle(name, x, cotangents, n=None, dtype=torch.float64, codes=None, counts=None, whole=False, sd=None):
    """The restatement's audio gradient on the CPU in `dtype`: of encode's outputs, or with whole=True of the eval forward's (the cotangent key
    "audio" then exists too)."""
    ref = DacRefE(config(name), state_dict(name) if sd is None else sd, dtype)
    fn = ref.forward_dict if whole else ref.encode_dict
    return grad_of(lambda xt: fn(xt, n, _t(codes), _t(counts)), x, cotangents, dtype)


def oracle_codes(name, x, n=None, dtype=torch.float64):
    """The codes the restatement chooses in `dtype` (no forcing)."""
    ref = DacRefE(config(name), state_dict(name), dtype)
    with torch.no_grad():
        return ref.encode_dict(torch.from_numpy(np.array(x)).to(dtype), n)["codes"].numpy()
