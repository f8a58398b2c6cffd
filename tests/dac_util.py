"""Our own torch restatement of the DAC baseline's eval path (reference: baselines/descript/dac/model/dac.py, nn/layers.py, nn/quantize.py),
written from a state_dict and a configuration with plain torch.nn.functional calls.  On the CPU it is pinned to the reference's fixtures
(tests/golden/dac_*.npz, tools/gen_dac_golden.py); on the GPU it is the oracle for wider sweeps and the PyTorch-eager baseline of
tools/dac_timing.py.  `quantize` can be forced to take given codes at given (row, stage) positions, so that a test can continue the
reference's search from the device's choice after a near-tie."""
import math

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN_NS = (1, 2, 6, 12, 18, None)


def nkey(n):
    return "nall" if n is None else f"n{n}"


def full_config(cfg):
    c = dict(encoder_dim=64, encoder_rates=[2, 4, 8, 8], latent_dim=None, decoder_dim=1536, decoder_rates=[8, 8, 4, 2], n_codebooks=9,
             codebook_size=1024, codebook_dim=8, sample_rate=44100)
    c.update({k: v for k, v in cfg.items() if k != "quantizer_dropout"})
    if c["latent_dim"] is None:
        c["latent_dim"] = c["encoder_dim"] * 2 ** len(c["encoder_rates"])
    return c


def snake(x, alpha):
    return x + (alpha + 1e-9).reciprocal() * torch.sin(alpha * x).pow(2)


class DacRef:
    """DAC eval forward from a state_dict (any device; fp32)."""

    def __init__(self, cfg, sd):
        self.cfg = full_config(cfg)
        self.sd = {k: v.float() for k, v in sd.items()}
        self.hop = int(np.prod(self.cfg["encoder_rates"]))

    def _w(self, p, dim=0):
        return torch._weight_norm(self.sd[p + "weight_v"], self.sd[p + "weight_g"], dim)

    def _conv(self, x, p, **kw):
        return F.conv1d(x, self._w(p), self.sd[p + "bias"], **kw)

    def _snake(self, x, p):
        return snake(x, self.sd[p + "alpha"])

    def _res(self, x, p, dil):
        y = self._conv(self._snake(x, p + "block.0."), p + "block.1.", dilation=dil, padding=3 * dil)
        y = self._conv(self._snake(y, p + "block.2."), p + "block.3.")
        assert y.shape[-1] == x.shape[-1]
        return x + y

    def encoder(self, x):
        r = self.cfg["encoder_rates"]
        x = self._conv(x, "encoder.block.0.", padding=3)
        for i, s in enumerate(r):
            p = f"encoder.block.{i + 1}.block."
            for j, d in enumerate((1, 3, 9)):
                x = self._res(x, f"{p}{j}.", d)
            x = self._conv(self._snake(x, f"{p}3."), f"{p}4.", stride=s, padding=math.ceil(s / 2))
        n = len(r)
        return self._conv(self._snake(x, f"encoder.block.{n + 1}."), f"encoder.block.{n + 2}.", padding=1)

    def decoder(self, z):
        r = self.cfg["decoder_rates"]
        x = self._conv(z, "decoder.model.0.", padding=3)
        for i, s in enumerate(r):
            p = f"decoder.model.{i + 1}.block."
            x = self._snake(x, f"{p}0.")
            x = F.conv_transpose1d(x, self._w(f"{p}1."), self.sd[f"{p}1.bias"], stride=s, padding=math.ceil(s / 2))
            for j, d in enumerate((1, 3, 9)):
                x = self._res(x, f"{p}{j + 2}.", d)
        n = len(r)
        return torch.tanh(self._conv(self._snake(x, f"decoder.model.{n + 1}."), f"decoder.model.{n + 2}.", padding=3))

    def _codebook_search(self, i, ze):
        """(B, d, T) latents -> (dist (B*T, K), indices (B, T)), quantize.py:88-109."""
        enc = F.normalize(ze.transpose(1, 2).reshape(-1, ze.shape[1]))
        cb = F.normalize(self.sd[f"quantizer.quantizers.{i}.codebook.weight"])
        dist = enc.pow(2).sum(1, keepdim=True) - 2 * enc @ cb.t() + cb.pow(2).sum(1, keepdim=True).t()
        return dist, (-dist).max(1)[1].reshape(ze.shape[0], ze.shape[2])

    def quantize(self, z, n=None, force=None, margins=False):
        """ResidualVectorQuantize.forward in eval mode (quantize.py:127-198).  force: {(row, stage): code} with row = b * T + t.
        Returns z_q, codes, latents, commitment_loss, codebook_loss, margins: with margins=True (B, n, T) second-best minus best distance
        (work the reference does not do: off for timing), else None."""
        want_margins = margins
        nc = self.cfg["n_codebooks"]
        n = nc if n is None else min(n, nc)
        B, _, T = z.shape
        zq, residual = 0, z
        cm = cb = 0
        codes, lats, margins = [], [], []
        for i in range(n):
            p = f"quantizer.quantizers.{i}."
            ze = self._conv(residual, p + "in_proj.")
            dist, idx = self._codebook_search(i, ze)
            if force:
                flat = idx.reshape(-1).clone()
                for (row, st), c in force.items():
                    if st == i:
                        flat[row] = c
                idx = flat.reshape(B, T)
            if want_margins:
                top2 = torch.topk(dist, 2, dim=1, largest=False).values
                margins.append((top2[:, 1] - top2[:, 0]).reshape(B, T))
            q = F.embedding(idx, self.sd[p + "codebook.weight"]).transpose(1, 2)
            cm_i = F.mse_loss(ze, q, reduction="none").mean([1, 2])
            cb_i = F.mse_loss(q, ze, reduction="none").mean([1, 2])
            q = ze + (q - ze)
            q = self._conv(q, p + "out_proj.")
            zq = zq + q
            residual = residual - q
            cm = cm + cm_i.mean()
            cb = cb + cb_i.mean()
            codes.append(idx)
            lats.append(ze)
        return zq, torch.stack(codes, 1), torch.cat(lats, 1), cm, cb, (torch.stack(margins, 1) if want_margins else None)

    def from_codes(self, codes):
        zq, zp = 0.0, []
        for i in range(codes.shape[1]):
            p = f"quantizer.quantizers.{i}."
            zpi = F.embedding(codes[:, i], self.sd[p + "codebook.weight"]).transpose(1, 2)
            zp.append(zpi)
            zq = zq + self._conv(zpi, p + "out_proj.")
        return zq, torch.cat(zp, 1), codes

    def encode(self, x, n=None):
        return self.quantize(self.encoder(x), n)[:5]

    def forward(self, x, n=None):
        L = x.shape[-1]
        x = F.pad(x, (0, math.ceil(L / self.hop) * self.hop - L))
        z, codes, lat, cm, cb = self.encode(x, n)
        return {"audio": self.decoder(z)[..., :L], "z": z, "codes": codes, "latents": lat, "vq/commitment_loss": cm, "vq/codebook_loss": cb}


def num_frames(cfg, L):
    """Latent frames of an L-sample clip: torch's Conv1d length formula through every encoder layer."""
    c = full_config(cfg)
    t = L                                   # first conv: k 7, pad 3 keeps the length
    for s in c["encoder_rates"]:
        t = (t + 2 * math.ceil(s / 2) - 2 * s) // s + 1
    return t


def output_samples(cfg, T):
    """Samples decoded from T latent frames: ConvTranspose1d's (T - 1) * s - 2 p + k per decoder block."""
    c = full_config(cfg)
    for s in c["decoder_rates"]:
        T = (T - 1) * s - 2 * math.ceil(s / 2) + 2 * s
    return T


def attribute_codes(ref: DacRef, z, n, got, want, margins, tol=2e-6):
    """The project's near-tie rule.  got / want: (B, n, T) codes (device / reference).  A row may differ from the reference only where the
    reference's margin at its EARLIEST differing stage is below tol; the later stages of such a row must equal the restatement continued from
    the device's choice there.  Returns (number of attributed rows, list of violations)."""
    got = np.asarray(got); want = np.asarray(want); margins = np.asarray(margins)
    B, S, T = want.shape
    force, bad, rows = {}, [], 0
    for b in range(B):
        for t in range(T):
            d = np.nonzero(got[b, :, t] != want[b, :, t])[0]
            if not len(d):
                continue
            s = int(d[0])
            if margins[b, s, t] >= tol:
                bad.append((b, s, t, float(margins[b, s, t])))
                continue
            force[(b * T + t, s)] = int(got[b, s, t])
            rows += 1
    if force and not bad:
        for _ in range(S):                  # a continued row may meet a second near-tie later on: follow the device there too
            cont = ref.quantize(z, n, force=force, margins=True)
            c2, m2 = cont[1].cpu().numpy(), cont[5].cpu().numpy()
            new = False
            for b in range(B):
                for t in range(T):
                    d = np.nonzero(got[b, :, t] != c2[b, :, t])[0]
                    if not len(d):
                        continue
                    s = int(d[0])
                    if m2[b, s, t] >= tol or (b * T + t, s) in force:
                        bad.append((b, s, t, float(m2[b, s, t])))
                    else:
                        force[(b * T + t, s)] = int(got[b, s, t]); new = True
            if bad or not new:
                break
    return rows, bad
