"""CPU restatement of the rvq+swinT codec (RVQCodecs, codecs.py:96-181) for tests/test_rvq.py: the encoder, decoder blocks and codebook
search of oracle/esc_oracle.py (imported unchanged) around the bottleneck product-residual quantiser (quantization.py:139-431) stated here,
plus the code-parity rule of that quantiser."""
import json

import numpy as np
import torch
import torch.nn.functional as F

from conftest import load_golden, synth_state
from oracle.esc_oracle import (EscOracle, audio_reconstruct, codebook_search, patch_deembed, pvq_frames, pvq_unframes, spec_transform,
                               split_dimension, transformer_layer)

NEAR_TIE = 2e-6          # reference margin below which a device argmin flip is fp32 re-association noise (tests/gpu_util.py NEAR_TIE)


def esc_config(cfg: dict) -> dict:
    """The backbone's configuration in EscOracle's terms (RVQCodecs kwargs minus the quantiser's own)."""
    out = {k: v for k, v in cfg.items() if k not in ("num_rvqs", "codebook_dim")}
    out["codebook_dims"] = [cfg["codebook_dim"]] * cfg["max_streams"]
    return out


class RvqOracle:
    def __init__(self, cfg: dict, sd):
        self.cfg = dict(cfg)
        self.orc = EscOracle(esc_config(cfg), sd)
        self.sd = self.orc.sd
        c = self.orc.cfg
        self.G, self.R, self.d = cfg["group_size"], cfg["num_rvqs"], cfg["codebook_dim"]
        self.ov, self.l2 = c["overlap"], c["l2norm"]
        self.Hq = c["in_freq"] // c["patch_size"][0] // 2 ** (c["max_streams"] - 1)     # base.py:78-80
        self.dims = split_dimension(self.ov * self.Hq * c["h_dims"][-1], self.G)

    def cb(self, m, i):
        return self.sd[f"quantizers.vqs.{m}.vqs.{i}.embedding.weight"]

    def project(self, tokens):
        """bottleneck tokens (B, Hq*W, C) -> projected vectors (B, T, G, d) (quantization.py:367-372)."""
        v = pvq_frames(tokens, self.Hq, self.ov)
        out, s = [], 0
        for m in range(self.G):
            out.append(F.linear(v[..., s:s + self.dims[m]], self.sd[f"quantizers.vqs.{m}.proj_down.weight"]))
            s += self.dims[m]
        return torch.stack(out, dim=2)

    def quantize(self, z, S, force=None):
        """z (B, T, G, d) -> codes (B, S', G, T), margins (B, S', G, T), cm_loss (B,) with S' = min(S, num_rvqs) (quantization.py:167-203,
        230-243, 337-338).  force: (B, S', G, T) int64, -1 = free: codes imposed on the search (continuation after a near-tie)."""
        B, T = z.shape[:2]
        S = min(S, self.R)
        codes = torch.empty((B, S, self.G, T), dtype=torch.int64)
        margins = torch.empty((B, S, self.G, T))
        loss = torch.zeros(B)
        for m in range(self.G):
            r = z[:, :, m, :]
            for i in range(S):
                idx, mg = codebook_search(r.reshape(B * T, -1), self.cb(m, i), self.l2, want_margin=True)
                idx = idx.view(B, T)
                if force is not None:
                    idx = torch.where(force[:, i, m] >= 0, force[:, i, m], idx)
                e = F.embedding(idx, self.cb(m, i))
                loss = loss + F.mse_loss(e, r, reduction="none").mean([1, 2])
                r = r - e
                codes[:, i, m], margins[:, i, m] = idx, mg.view(B, T)
        return codes, margins, loss / self.G

    def dequantize(self, codes):
        """codes (B, S, G, T) -> decoder input tokens (B, Hq*W, C): proj_up of the SUM of the raw rows (quantization.py:283-289, 406-420)."""
        parts = []
        for m in range(self.G):
            zq = 0.
            for i in range(codes.shape[1]):
                zq = zq + F.embedding(codes[:, i, m], self.cb(m, i))
            parts.append(F.linear(zq, self.sd[f"quantizers.vqs.{m}.proj_up.weight"]))
        return pvq_unframes(torch.cat(parts, dim=-1), self.Hq, self.ov)

    def decode_tokens(self, zq, feat_shape):
        """Decoder.forward (base.py:195-203) + ISTFT."""
        c = self.orc.cfg
        H, W = feat_shape
        for i in range(len(c["h_dims"]) - 1):
            zq, H, W = self.orc._dec_block(i, zq, H, W)
        zq, H, W = transformer_layer(zq, H, W, self.sd, "decoder.post_nn.", self.orc.dec_heads[-1], c["swin_depth"], c["window_size"], None)
        feat = patch_deembed(zq, H, self.sd, "decoder.patch_deembed.", c["patch_size"])
        return audio_reconstruct(feat, c, self.sd.get("ift.window"))

    @torch.no_grad()
    def bottleneck(self, x):
        feat = spec_transform(x, self.orc.cfg, self.sd.get("ft.window"))
        enc_hs, shape = self.orc.encoder(feat)
        return enc_hs[-1], shape

    @torch.no_grad()
    def encode(self, x, S):
        tok, shape = self.bottleneck(x)
        codes, _, _ = self.quantize(self.project(tok), S)
        return codes, shape

    @torch.no_grad()
    def decode(self, codes, feat_shape):
        return self.decode_tokens(self.dequantize(codes), feat_shape)


def load(name):
    """(RvqOracle, golden npz, cfg, state dict) for tests/golden/{name}.npz."""
    g = load_golden(name)
    cfg = json.loads(str(g["config_json"]))
    sd = synth_state(name)
    return RvqOracle(cfg, sd), g, cfg, sd


def continue_vector(orc, z, m, first):
    """Codes of stages len(first).. of one (vector, group) when stages 0..len(first)-1 are forced to `first` (z: (d,) projected vector)."""
    r = z.clone()
    out = []
    for i in range(orc.R):
        idx, mg = codebook_search(r[None], orc.cb(m, i), orc.l2, want_margin=True)
        k = int(first[i]) if i < len(first) else int(idx[0])
        out.append((k, float(mg[0])))
        r = r - orc.cb(m, i)[k]
    return out


def attribute(orc, got, ref, margins, z, tol=NEAR_TIE):
    """The parity rule of the product-residual quantiser.  got / ref (B, S, G, T); margins (B, R, G, T) and z (B, T, G, d) from the fixture.
    A flip changes only the later stages of its own (vector, group): where got and ref differ, the earliest differing stage must be a reference
    near-tie, and every later stage must equal the restatement continued from the device's codes on the fixture's projected vector (a further
    difference there must itself be a near-tie of the continued search).  Returns the list of unattributable (b, g, t, stage)."""
    got = np.asarray(got); ref = np.asarray(ref)
    bad = []
    diff = (got != ref).any(axis=1)
    for b, g, t in np.argwhere(diff):
        col, rcol = got[b, :, g, t], ref[b, :, g, t]
        i = int(np.argmax(col != rcol))
        if not margins[b, i, g, t] < tol:
            bad.append((int(b), int(g), int(t), i))
            continue
        zt = torch.from_numpy(np.ascontiguousarray(z[b, t, g]))
        forced = list(col[: i + 1])
        while len(forced) < len(col):
            cont = continue_vector(orc, zt, g, forced)
            j = len(forced)
            k, mg = cont[j]
            if k != col[j] and not mg < tol:
                bad.append((int(b), int(g), int(t), j))
                break
            forced.append(col[j])
    return bad
