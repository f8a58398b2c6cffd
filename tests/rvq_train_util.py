"""Differentiable CPU restatement of the rvq+swinT TRAINING step (RVQCodecs.forward in training mode, codecs.py:127-167) for
tests/test_rvq_train*.py: tests/rvq_util.py's RvqOracle (encoder, decoder blocks and codebook search of oracle/esc_oracle.py, imported unchanged)
around the training form of the product-residual quantiser (quantization.py:167-196, 298-335; codebook.py:57-75) under plain autograd, the
trainer's losses of oracle/esc_oracle.py, and the comparison helpers of tests/test_train.py (copied, not imported from a test module)."""
import json

import numpy as np
import torch
import torch.nn.functional as F

from conftest import load_golden, synth_state
from esc import synth
from oracle import esc_oracle as O
from rvq_util import RvqOracle, esc_config

LOSS_RTOL = 1e-5
GRAD_TOL = 1e-4
MIN_MARGIN = 1e-5        # five times rvq_util.NEAR_TIE: the inputs of every device comparison leave the reference's own search this much room


def cfg_of(name):
    return json.loads(str(load_golden(name)["config_json"]))


def fixture_clips(g, name):
    tags = json.loads(str(g[f"{name}_tags"]))
    n = json.loads(str(g["n_samples_json"]))[name]
    pcm = np.stack([synth.noise_clip_int16(tags[0], n), synth.voiced_clip_int16(tags[1], n)])
    return torch.from_numpy(synth.pcm_to_float(pcm))


# Clips for shapes without a fixture, chosen with tools/gen_rvq_golden.py pick's rule (of six candidate tags per kind, the largest smallest margin of the
# restatement's training forward at that length; smallest here 5.6e-4).  The tests still assert MIN_MARGIN on the restatement before they look at the device.
SHAPE_TAGS = {("rvq_tiny", 1180): ["rvq-train-noise-0", "rvq-train-voiced-3", "rvq-train-noise-4"],
              ("rvq_base", 5040): ["rvq-train-noise-0", "rvq-train-voiced-1", "rvq-train-noise-2"],
              ("rvq_base", 3440): ["rvq-train-noise-2", "rvq-train-voiced-1", "rvq-train-noise-5"]}


def shape_clips(name, B, L):
    tags = SHAPE_TAGS[(name, L)][:B]
    pcm = np.stack([(synth.voiced_clip_int16 if "voiced" in t else synth.noise_clip_int16)(t, L) for t in tags])
    return torch.from_numpy(synth.pcm_to_float(pcm))


class RvqTrainOracle(RvqOracle):
    """RvqOracle on leaf tensors (keep_graph) with the training-mode forward."""

    def __init__(self, cfg, sd):
        super().__init__(cfg, sd)
        self.orc = O.EscOracle(esc_config(cfg), sd, keep_graph=True)
        self.sd = self.orc.sd

    def quantize_train(self, z, S, freeze, force=None):
        """z (B, T, G, d) -> operand of the up-projections (B, T, G, d), codes (B, R, G, T), margins (B, R, G, T), cm, cb (B,).
        The stage arithmetic of quantization.py:178-193 with codebook.py:64-70, literally; force (B, R, G, T) int64, -1 = free."""
        B, T = z.shape[:2]
        codes = torch.empty((B, self.R, self.G, T), dtype=torch.int64)
        margins = torch.empty((B, self.R, self.G, T), dtype=z.dtype)
        outs, cm_loss, cb_loss = [], 0.0, 0.0
        for m in range(self.G):
            ze = z[:, :, m, :]
            r, zq, cm_m, cb_m = ze, 0.0, 0.0, 0.0
            for i in range(self.R):
                cbw = self.cb(m, i)
                idx, mg = O.codebook_search(r.detach().reshape(B * T, -1), cbw.detach(), self.l2, want_margin=True)
                idx = idx.view(B, T)
                if force is not None:
                    idx = torch.where(force[:, i, m] >= 0, force[:, i, m], idx)
                q = F.embedding(idx, cbw)
                cm = F.mse_loss(q.detach(), r, reduction="none").mean([1, 2])          # codebook.py:68
                cb = F.mse_loss(q, r.detach(), reduction="none").mean([1, 2])          # codebook.py:69
                zi = r + (q - r).detach()                                              # codebook.py:70
                r = r - zi                                                             # quantization.py:184
                if i >= S:                                                             # quantization.py:185-187
                    zi = zi * 0.0
                    cm, cb = cm * 0.0, cb * 0.0
                zq = zq + zi
                cm_m, cb_m = cm_m + cm, cb_m + cb
                codes[:, i, m], margins[:, i, m] = idx, mg.view(B, T)
            if freeze:                                                                 # quantization.py:319-321
                zq = ze + zq * 0.0
                cm_m, cb_m = cm_m * 0.0, cb_m * 0.0
            outs.append(zq)
            cm_loss, cb_loss = cm_loss + cm_m, cb_loss + cb_m
        return torch.stack(outs, dim=2), codes, margins, cm_loss / self.G, cb_loss / self.G

    def forward_train(self, x, S, freeze=False, force=None, x_feat=None):
        c = self.orc.cfg
        feat = O.spec_transform(x, c, self.sd.get("ft.window")) if x_feat is None else x_feat.permute(0, 3, 1, 2)
        enc_hs, shape = self.orc.encoder(feat)
        z = self.project(enc_hs[-1])
        zq, codes, margins, cm, cb = self.quantize_train(z, min(S, self.R), freeze, force)
        parts = [F.linear(zq[:, :, m, :], self.sd[f"quantizers.vqs.{m}.proj_up.weight"]) for m in range(self.G)]
        tok = O.pvq_unframes(torch.cat(parts, dim=-1), self.Hq, self.ov)
        H, W = shape
        for i in range(len(c["h_dims"]) - 1):
            tok, H, W = self.orc._dec_block(i, tok, H, W)
        tok, H, W = O.transformer_layer(tok, H, W, self.sd, "decoder.post_nn.", self.orc.dec_heads[-1], c["swin_depth"], c["window_size"], None)
        recon_feat = O.patch_deembed(tok, H, self.sd, "decoder.patch_deembed.", c["patch_size"])
        return {"cm_loss": cm, "cb_loss": cb, "raw_audio": x, "recon_audio": O.audio_reconstruct(recon_feat, c, self.sd.get("ift.window")),
                "raw_feat": feat, "recon_feat": recon_feat, "codes": codes, "margins": margins.detach(), "z_e": z, "z_q": zq}


def oracle_step(name, S, freeze, x, dtype=torch.float32, smooth=None, weights=None, force=None, input_grad=False, x_feat=None):
    """One training step of the restatement under autograd.  smooth = (A, R, wc, wb): the smooth functional of tests/test_train.py
    (mean_b[wc cm + wb cb + <recon_audio, A> + <recon_feat, R>]); otherwise the trainer's losses with `weights`.  Returns (out, losses, grads);
    with input_grad, grads["__input__"] is d scalar / d x (or d x_feat)."""
    sd = {k: (v.to(dtype).clone().requires_grad_(True) if (v.is_floating_point() and not k.endswith(".window")) else
              (v.to(dtype) if v.is_floating_point() else v)) for k, v in synth_state(name).items()}
    orc = RvqTrainOracle(cfg_of(name), sd)
    xin = x.detach().to(dtype).clone()
    fin = None if x_feat is None else x_feat.detach().to(dtype).clone()
    if input_grad:
        (fin if fin is not None else xin).requires_grad_(True)
    out = orc.forward_train(xin, S, freeze, force=force, x_feat=fin)
    if smooth is None:
        ls = O.training_loss(out, weights or O.LOSS_WEIGHTS)
    else:
        A, R, wc, wb = smooth
        total = out["cm_loss"] * wc + out["cb_loss"] * wb + (out["recon_audio"] * A.to(dtype)).sum(1) + (out["recon_feat"] * R.to(dtype)).sum((1, 2, 3))
        ls = {"loss": total, "scalar": total.mean()}
    ls["scalar"].backward()
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in sd.items() if v.is_floating_point() and v.requires_grad}
    if input_grad:
        grads["__input__"] = (fin if fin is not None else xin).grad
    return out, ls, grads


def product_model(name):
    from esc.models import make_model
    model = make_model(cfg_of(name), "rvq+swinT")
    model.load_state_dict(synth_state(name))
    return model.cuda().train()


def product_step(name, S, freeze, x, w=None, smooth=None, x_feat=None, model=None, input_grad=False):
    """The same step through esc.RVQCodecs in train mode (libescx escx_rvq_train_forward / escx_rvq_train_backward and the HIP loss modules)."""
    from esc.modules import ComplexSTFTLoss, MelSpectrogramLoss
    if model is None:
        model = product_model(name)
    else:
        model.zero_grad(set_to_none=True)          # a reused model starts from empty gradients, like a fresh one
    xin = x.detach().cuda().clone()
    fin = None if x_feat is None else x_feat.detach().cuda().clone()
    if input_grad:
        (fin if fin is not None else xin).requires_grad_(True)
    out = model(**dict(x=xin, x_feat=fin, num_streams=S, freeze_codebook=freeze))
    losses = {"cm": out["cm_loss"].detach().cpu().numpy(), "cb": out["cb_loss"].detach().cpu().numpy()}
    if smooth is None:
        mel = MelSpectrogramLoss()(out["raw_audio"], out["recon_audio"])
        stft = ComplexSTFTLoss()(out["raw_feat"], out["recon_feat"])
        loss = out["cm_loss"] * w["cm_weight"] + out["cb_loss"] * w["cb_weight"] + mel * w["mel_weight"] + stft * w["stft_weight"]
        losses.update(mel=mel.detach().cpu().numpy(), stft=stft.detach().cpu().numpy())
    else:
        A, R, wc, wb = smooth
        loss = out["cm_loss"] * wc + out["cb_loss"] * wb + (out["recon_audio"] * A.cuda()).sum(1) + (out["recon_feat"] * R.cuda()).sum((1, 2, 3))
    loss.mean().backward()
    torch.cuda.synchronize()
    grads = {k: (p.grad.detach().cpu().numpy() if p.grad is not None else np.zeros(tuple(p.shape), np.float32)) for k, p in model.named_parameters()}
    if input_grad:
        grads["__input__"] = (fin if fin is not None else xin).grad.detach().cpu().numpy()
    losses["loss"] = loss.detach().cpu().numpy()
    return model, out, losses, grads


def smooth_probe(name, x, wc=0.7, wb=1.3, vq_only=False):
    """Fixed random cotangents for recon_audio / recon_feat (different per clip) and VQ-loss weights (tests/test_train.py _smooth_probe);
    vq_only: weight on cm and cb alone."""
    cfg = cfg_of(name)
    g = torch.Generator().manual_seed(77)
    hop = int(cfg["hop_len"] * cfg["sr"] * 1e-3)
    T = 1 + x.shape[1] // hop
    A = torch.randn(x.shape[0], hop * ((T // 2) * 2 - 1), generator=g) / x.shape[1]
    R = torch.randn(x.shape[0], 2, cfg["in_freq"], (T // 2) * 2, generator=g) / (cfg["in_freq"] * T)
    if vq_only:
        A, R = torch.zeros_like(A), torch.zeros_like(R)
    return A, R, wc, wb


def rel_rms(a, b, floor):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.sqrt(np.mean((a - b) ** 2)) / max(float(np.sqrt(np.mean(b ** 2))), floor))


def grad_scale(grads):
    return float(np.sqrt(sum(float((torch.as_tensor(v).double() ** 2).sum()) for k, v in grads.items() if k != "__input__")))


def check_grads(got, ref, tol, what):
    """Every parameter gradient within `tol` relative RMS of the restatement's (floor: 1e-6 of the whole gradient's norm, spread over the elements)."""
    scale = grad_scale(ref)
    worst = (0.0, "")
    for k, r in ref.items():
        r = r.numpy() if torch.is_tensor(r) else r
        floor = 1e-6 * scale / np.sqrt(r.size) if k != "__input__" else 1e-12
        err = rel_rms(got[k], r, floor)
        worst = max(worst, (err, k))
        assert err <= tol, f"{what}: gradient of {k} rel rms {err:.3e} (|ref| {np.linalg.norm(r):.3e})"
    return worst


def check_against_fixture(g, tag, keys, losses, codes, grads, grad_tol):
    for k in ("cm", "cb", "mel", "stft", "loss"):
        np.testing.assert_allclose(losses[k], g[f"{tag}_{k}"], rtol=LOSS_RTOL, atol=1e-7, err_msg=f"{tag} {k}")
    assert np.array_equal(np.asarray(codes), g[f"{tag}_codes"].astype(np.int64)), f"{tag}: codes differ from the reference"
    ref_norm = g[f"{tag}_gnorm"]
    scale = float(np.sqrt((ref_norm ** 2).sum()))
    for k, rn in zip(keys, ref_norm):
        gn = float(np.linalg.norm(np.asarray(grads[k], np.float64)))
        assert abs(gn - rn) <= grad_tol * max(rn, 1e-6 * scale) + 1e-12, f"{tag}: |grad {k}| = {gn} vs reference {rn}"
    for key in [f for f in g.files if f.startswith(f"{tag}_g::")]:
        k = key.split("::", 1)[1]
        ref = g[key]
        floor = 1e-6 * scale / np.sqrt(ref.size)
        err = rel_rms(grads[k], ref, floor)
        assert err <= grad_tol, f"{tag}: gradient of {k} rel rms {err:.3e}"
        if not ref.any():
            assert not np.asarray(grads[k]).any(), f"{tag}: gradient of {k} must be exactly zero"


def noise_floor(name, S, freeze, x, weights, force, draws=3):
    """tests/test_train.py _noise_floor for the rvq restatement: per-parameter relative RMS distance between fp32 evaluations of the restatement and its
    fp64 gradients of the trainer's loss (codes forced to the fp32 run's), envelope over `draws` realisations (default run, inputs moved by one ulp with
    random signs, default inputs summed single-threaded)."""
    _, _, g64 = oracle_step(name, S, freeze, x, dtype=torch.float64, weights=weights, force=force)
    scale = grad_scale(g64)
    gen = torch.Generator().manual_seed(5)
    floor, medians = {k: 0.0 for k in g64}, []
    for d in range(draws):
        nt = torch.get_num_threads()
        xd = x if d != 1 else x * (1 + (torch.randint(0, 2, x.shape, generator=gen).float() * 2 - 1) * 2.0 ** -23)
        if d == 2:
            torch.set_num_threads(1)
        try:
            _, _, g32 = oracle_step(name, S, freeze, xd, weights=weights, force=force)
        finally:
            torch.set_num_threads(nt)
        e = {k: rel_rms(g32[k].numpy(), g64[k].numpy(), 1e-6 * scale / np.sqrt(g64[k].numel())) for k in g64}
        medians.append(float(np.median(list(e.values()))))
        floor = {k: max(floor[k], e[k]) for k in g64}
    return g64, floor, scale, max(medians)
