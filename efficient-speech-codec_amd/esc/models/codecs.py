"""esc.ESC -- host side of the MI355X-native ESC codec.

Keeps the reference's Python surface (`/root/reference/esc/models/codecs.py:9-94,183-200`): the constructor
kwargs, `.encode(x, num_streams) -> (codes, feat_shape)`, `.decode(codes, feat_shape) -> wave`, the eval-mode
`.forward(x, x_feat, num_streams)` dict, `max_streams`, `max_bps`, `make_model`, and the reference state_dict
key layout (so reference checkpoints load with `load_state_dict`).  The parameters live here as ordinary
`nn.Parameter`s; the arithmetic lives in libescx.so (hand-written HIP for gfx950) reached through ctypes.
There is NO PyTorch/CPU implementation of the path in this package: a CPU tensor or a missing library raises.
"""
from __future__ import annotations

import ctypes
import math
import operator
from typing import Dict, List, Literal, Optional, Tuple

import torch
import torch.nn as nn

from .. import _native

__all__ = ["ESC", "RVQCodecs", "make_model", "model_dict", "state_manifest", "rvq_state_manifest"]


def _rel_pos_index(ws: int) -> torch.Tensor:
    """(dh+ws-1)*(2ws-1) + (dw+ws-1); reference attention.py:195-205."""
    ih = torch.arange(ws).repeat_interleave(ws)
    iw = torch.arange(ws).repeat(ws)
    return ((ih[:, None] - ih[None, :] + ws - 1) * (2 * ws - 1) + (iw[:, None] - iw[None, :] + ws - 1)).long()


def state_manifest(cfg: dict) -> Dict[str, Tuple[int, ...]]:
    """key -> shape of the reference state_dict for this configuration."""
    h, heads, depth, ws = list(cfg["h_dims"]), list(cfg["swin_heads"]), cfg["swin_depth"], cfg["window_size"]
    n, S, G = len(h), cfg["max_streams"], cfg["group_size"]
    pf, pt = cfg["patch_size"]
    win = int(cfg["win_len"] * cfg["sr"] * 1e-3)
    man: Dict[str, Tuple[int, ...]] = {"ft.window": (win,), "ift.window": (win,)}
    dec = h[::-1]
    H0 = cfg["in_freq"] // pf
    for s in range(S):                                                  # base.py:49-69
        C = dec[max(s - 1, 0)]
        Hq = H0 // 2 ** (S - 1) if s == 0 else H0 // 2 ** (S - s)
        D = cfg["overlap"] * Hq * C
        dims = [D // G] * G
        dims[-1] = D - (D // G) * (G - 1)
        d = cfg["codebook_dims"][s]
        for g in range(G):
            man[f"quantizers.{s}.vqs.{g}.embedding.weight"] = (cfg["codebook_size"], d)
        for g in range(G):
            man[f"quantizers.{s}.down_projs.{g}.weight"] = (d, dims[g])
        for g in range(G):
            man[f"quantizers.{s}.up_projs.{g}.weight"] = (dims[g], d)

    def block(p, C, nH):
        hid = int(C * cfg["mlp_ratio"])
        for j in range(depth):
            q = f"{p}swint_blocks.{j}."
            man[q + "norm1.weight"] = (C,); man[q + "norm1.bias"] = (C,)
            man[q + "attn.relative_position_bias_table"] = ((2 * ws - 1) ** 2, nH)
            man[q + "attn.relative_position_index"] = (ws * ws, ws * ws)
            man[q + "attn.qkv.weight"] = (3 * C, C); man[q + "attn.qkv.bias"] = (3 * C,)
            man[q + "attn.proj.weight"] = (C, C); man[q + "attn.proj.bias"] = (C,)
            man[q + "norm2.weight"] = (C,); man[q + "norm2.bias"] = (C,)
            man[q + "mlp.linear_1.weight"] = (hid, C); man[q + "mlp.linear_1.bias"] = (hid,)
            man[q + "mlp.linear_2.weight"] = (C, hid); man[q + "mlp.linear_2.bias"] = (C,)

    for i in range(n - 1):
        p = f"encoder.blocks.{i}."
        block(p, h[i], heads[i])
        man[p + "subsample.norm.weight"] = (2 * h[i],); man[p + "subsample.norm.bias"] = (2 * h[i],)
        man[p + "subsample.down.weight"] = (h[i + 1], 2 * h[i])
    man["encoder.patch_embed.proj.weight"] = (h[0], cfg["in_dim"], pf, pt)
    man["encoder.patch_embed.proj.bias"] = (h[0],)
    man["encoder.patch_embed.norm.weight"] = (h[0],); man["encoder.patch_embed.norm.bias"] = (h[0],)
    block("encoder.pre_nn.", h[0], heads[0])
    rh = heads[::-1]
    for j in range(n - 1):
        p = f"decoder.blocks.{j}."
        block(p, dec[j], rh[j])
        man[p + "subsample.norm.weight"] = (dec[j],); man[p + "subsample.norm.bias"] = (dec[j],)
        man[p + "subsample.up.weight"] = (2 * dec[j + 1], dec[j])
    man["decoder.patch_deembed.de_proj1.weight"] = (h[0] * pf * pt, h[0], 5, 5)
    man["decoder.patch_deembed.de_proj1.bias"] = (h[0] * pf * pt,)
    man["decoder.patch_deembed.de_proj2.weight"] = (cfg["in_dim"], h[0], 3, 3)
    man["decoder.patch_deembed.de_proj2.bias"] = (cfg["in_dim"],)
    block("decoder.post_nn.", dec[-1], rh[-1])
    return man


def _split_dimension(total: int, num: int) -> List[int]:
    """quantization.py:380-386: equal slices, the remainder goes to the last one."""
    dims = [total // num] * num
    dims[-1] = total - (total // num) * (num - 1)
    return dims


def rvq_state_manifest(cfg: dict) -> Dict[str, Tuple[int, ...]]:
    """key -> shape of the reference RVQCodecs state_dict (codecs.py:96-127): ESC's backbone keys and, at the bottleneck, one
    ResidualVectorQuantize per product group (base.py:73-84, quantization.py:139-164, 292-315)."""
    S, G, d = cfg["max_streams"], cfg["group_size"], cfg["codebook_dim"]
    base = state_manifest(dict(cfg, codebook_dims=[d] * S))
    man: Dict[str, Tuple[int, ...]] = {"ft.window": base["ft.window"], "ift.window": base["ift.window"]}
    Hq = cfg["in_freq"] // cfg["patch_size"][0] // 2 ** (S - 1)
    for m, dm in enumerate(_split_dimension(cfg["overlap"] * Hq * cfg["h_dims"][-1], G)):
        p = f"quantizers.vqs.{m}."
        man[p + "proj_down.weight"] = (d, dm)
        man[p + "proj_up.weight"] = (dm, d)
        for i in range(cfg["num_rvqs"]):
            man[p + f"vqs.{i}.embedding.weight"] = (cfg["codebook_size"], d)
    for k, v in base.items():
        if not k.startswith("quantizers.") and k not in man:
            man[k] = v
    return man


def _init_tensor(key: str, shape) -> torch.Tensor:
    """Default initialisation with the distributions the reference's modules use."""
    if key.endswith("relative_position_index"):
        return _rel_pos_index(int(math.isqrt(shape[0])))
    if key.endswith(".window"):
        return torch.hann_window(shape[0])
    t = torch.empty(shape)
    if ".norm" in key:
        return t.fill_(1.0) if key.endswith("weight") else t.zero_()
    if key.endswith("relative_position_bias_table"):
        return nn.init.trunc_normal_(t, std=0.02)                       # attention.py:212
    if key.endswith("embedding.weight"):
        return nn.init.kaiming_normal_(t)                               # codebook.py:14
    fan_in = shape[1] * (shape[2] * shape[3] if len(shape) == 4 else 1) if len(shape) > 1 else shape[0]
    bound = 1.0 / math.sqrt(max(fan_in, 1))
    return t.uniform_(-bound, bound)


class _Node(nn.Module):
    """Plain container so that parameters register under the reference's dotted key names."""


def _attach(root: nn.Module, key: str, tensor: torch.Tensor, buffer: bool):
    parts = key.split(".")
    mod = root
    for p in parts[:-1]:
        if p not in mod._modules:
            mod.add_module(p, _Node())
        mod = mod._modules[p]
    if buffer:
        mod.register_buffer(parts[-1], tensor, persistent=True)
    else:
        mod.register_parameter(parts[-1], nn.Parameter(tensor))


class ESC(nn.Module):
    """Efficient Speech Codec (cross-scale residual VQ + Swin transformers), MI355X-native execution."""

    def __init__(self, in_dim: int = 2, in_freq: int = 192, h_dims: list = [45, 72, 96, 144, 192, 384],
                 max_streams: int = 6, win_len: int = 20, hop_len: int = 5, sr: int = 16000,
                 patch_size: list = [3, 2], swin_heads: list = [3, 6, 12, 24, 24], swin_depth: int = 2,
                 window_size: int = 4, mlp_ratio: float = 4.,
                 overlap: int = 2, group_size: int = 3,
                 codebook_size: int = 1024, codebook_dims: list = [8, 8, 8, 8, 8, 8],
                 l2norm: bool = True, backbone: Literal['transformer', 'convolution'] = 'transformer',
                 kernel_size: list = [5, 2], conv_depth: int = 1) -> None:
        super().__init__()
        if backbone != "transformer":
            raise NotImplementedError("only backbone='transformer' (csvq+swinT) is implemented; the convolution "
                                      "backbone is an ablation outside the accelerated path")
        self.cfg = dict(in_dim=in_dim, in_freq=in_freq, h_dims=list(h_dims), max_streams=max_streams, win_len=win_len,
                        hop_len=hop_len, sr=sr, patch_size=list(patch_size), swin_heads=list(swin_heads),
                        swin_depth=swin_depth, window_size=window_size, mlp_ratio=float(mlp_ratio), overlap=overlap,
                        group_size=group_size, codebook_size=codebook_size, codebook_dims=list(codebook_dims),
                        l2norm=bool(l2norm), backbone=backbone)
        self.in_freq, self.in_dim = in_freq, in_dim                      # base.py:16-20
        self.max_streams = max_streams
        self.enc_h_dims = list(h_dims)
        self.dec_h_dims = list(h_dims)[::-1]
        self.win_length = int(win_len * sr * 1e-3)                       # base.py:23
        self.hop_length = int(hop_len * sr * 1e-3)                       # base.py:24
        self.max_bps = (2 / overlap) * max_streams * math.log2(codebook_size) * group_size // (20 * patch_size[1] // 2)  # base.py:70
        if codebook_size > 32768:
            raise NotImplementedError("codebook_size > 32768: code indices travel as int16 between ranks (esc/distributed.py)")
        if len(codebook_dims) < max_streams or len(swin_heads) < len(h_dims) - 1:
            raise ValueError("codebook_dims / swin_heads shorter than the number of streams / scales")

        for key, shape in self._state_manifest().items():
            is_buf = key.endswith("relative_position_index") or key.endswith(".window")
            _attach(self, key, _init_tensor(key, shape), is_buf)

        self._handles: Dict[int, ctypes.c_void_p] = {}
        self._flat: Dict[int, dict] = {}                 # per device: flat fp32 parameter buffer the nn.Parameters are views of
        self._packed_version: Dict[int, int] = {}        # parameter fingerprint the packed device layouts were derived from
        self._dirty = True
        self._flat_grad_mode = False
        self._carry: Dict[int, tuple] = {}               # flat gradient buffers that survive a handle rebuild (see _handle)
        self._precision = None                           # None = the library's default (ESCX_PRECISION, else "f16x2"); see set_precision

    def _state_manifest(self) -> Dict[str, Tuple[int, ...]]:
        return state_manifest(self.cfg)

    @property
    def _code_streams(self) -> int:
        """Largest stream count a call accepts (ESC: max_streams; RVQCodecs: num_rvqs)."""
        return self.max_streams

    def _create_handle(self, lib, idx: int, hd: ctypes.c_void_p):
        cc = self._c_config()
        _native.check(lib.escx_create(ctypes.byref(cc), idx, ctypes.byref(hd)))

    # the training step's entry points (`_TrainStep` is shared with RVQCodecs, which overrides these two and `_code_streams`)
    def _train_forward_call(self, lib, hd, flat, x, feat, B, n, S, freeze, codes, recon, raw_fm, recon_fm, cm, cb, stream):
        """n = samples of x, or frames of feat when the spectrum is given; every tensor argument is a ctypes pointer (or None)."""
        if feat is not None:
            return lib.escx_train_forward_feat(hd, flat, feat, B, n, S, freeze, codes, recon, recon_fm, cm, cb, stream)
        return lib.escx_train_forward(hd, flat, x, B, n, S, freeze, codes, recon, raw_fm, recon_fm, cm, cb, stream)

    def _train_backward_call(self, lib, hd, d_recon, d_recon_fm, d_raw, d_cm, d_cb, gflat, d_in, with_input, stream):
        if with_input:
            return lib.escx_train_backward_ex(hd, d_recon, d_recon_fm, d_raw, d_cm, d_cb, gflat, d_in, stream)
        return lib.escx_train_backward(hd, d_recon, d_recon_fm, d_cm, d_cb, gflat, stream)

    # ---- weight management ------------------------------------------------------------------
    def _apply(self, fn, *a, **k):
        self._dirty = True
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        sd = dict(state_dict)
        own = self.state_dict()
        for k in ("ft.window", "ift.window"):            # torchaudio buffers: optional in incoming checkpoints
            if k not in sd:
                sd[k] = own[k]
        for k in own:                                    # the index buffer is regenerated if absent
            if k.endswith("relative_position_index") and k not in sd:
                sd[k] = own[k]
        self._dirty = True
        return super().load_state_dict(sd, strict=strict, **kw)

    # ---- arithmetic of the inference path (include/escx.h escx_set_precision) -----------------------------
    def set_precision(self, mode: str) -> "ESC":
        """Operand form of the K = C contractions (MLPs, Q / K / V, PatchMerge / PatchSplit, PatchDeEmbed) of encode / decode / eval forward:
        "fp32" (fp32 MFMA, the reference's operand precision), "bf16x3" (every fp32 operand split exactly into three bf16 terms: fp32 results up to
        summation order), "f16x2" (two fp16 terms, range-safe, truncation ~1e-7: the default and the fastest).  fp32 accumulation in every mode.
        Not part of the reference's surface - the reference has one arithmetic (ATen fp32)."""
        if mode not in _native.PRECISIONS:
            raise ValueError(f"precision {mode!r}: expected one of {sorted(_native.PRECISIONS)}")
        self._precision = mode
        lib = _native.load()
        for hd in self._handles.values():
            _native.check(lib.escx_set_precision(hd, _native.PRECISIONS[mode]))
        return self

    @property
    def precision(self) -> str:
        """The mode in effect (of the first live handle; before any handle exists: what set_precision chose, or the library default)."""
        if self._handles:
            code = _native.load().escx_get_precision(next(iter(self._handles.values())))
            return {v: k for k, v in _native.PRECISIONS.items()}[code]
        import os
        return self._precision or {"0": "fp32", "3": "bf16x3", "2": "f16x2"}.get(os.environ.get("ESCX_PRECISION", "f16x2"), os.environ.get("ESCX_PRECISION", "f16x2"))

    def refresh_weights(self):
        """Force a re-pack (in-place updates are detected through autograd's version counters; this is for exotic writes, e.g. through
        raw pointers, that bypass them)."""
        self._packed_version = {}

    def _c_config(self) -> _native.EscxConfig:
        c = self.cfg
        cc = _native.EscxConfig()
        cc.in_dim, cc.in_freq, cc.n_scales = c["in_dim"], c["in_freq"], len(c["h_dims"])
        for i, v in enumerate(c["h_dims"]):
            cc.h_dims[i] = v
        cc.max_streams = c["max_streams"]
        cc.win_length, cc.hop_length = self.win_length, self.hop_length
        cc.patch_f, cc.patch_t = c["patch_size"]
        for i, v in enumerate(c["swin_heads"][:_native.MAX_SCALES]):
            cc.swin_heads[i] = v
        cc.swin_depth, cc.window_size, cc.mlp_ratio = c["swin_depth"], c["window_size"], c["mlp_ratio"]
        cc.overlap, cc.group_size, cc.codebook_size = c["overlap"], c["group_size"], c["codebook_size"]
        for i, v in enumerate(c["codebook_dims"][:_native.MAX_SCALES]):
            cc.codebook_dims[i] = v
        cc.l2norm = int(c["l2norm"])
        return cc

    # ---- flat parameter buffer (training step) ------------------------------------------------
    def _param_version(self) -> int:
        """Changes whenever a parameter is modified in place (optimizer.step, param.data.copy_, ...): autograd's version counters."""
        return sum(p._version for p in self.parameters())

    def _named_params(self) -> Dict[str, nn.Parameter]:
        return dict(self.named_parameters())

    def _ensure_flat(self, device: torch.device, lib, hd) -> torch.Tensor:
        """One contiguous fp32 device buffer holding every trainable parameter in the library's canonical order; the nn.Parameters
        become views into it (so optimizer steps update it in place and the library re-derives its packed layouts on the device
        without any host copy).  Re-established lazily after .to() / external re-assignment of a parameter's storage."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        st = self._flat.get(idx)
        params = self._named_params()
        if st is None:
            n = lib.escx_flat_param_count(hd)
            layout = [(lib.escx_flat_param_key(hd, i).decode(), int(lib.escx_flat_param_offset(hd, i)), int(lib.escx_flat_param_numel(hd, i)))
                      for i in range(n)]
            flat = torch.zeros(int(lib.escx_flat_param_total(hd)), dtype=torch.float32, device=device)
            st = {"flat": flat, "layout": layout}
            self._flat[idx] = st
        flat = st["flat"]
        base = flat.data_ptr()
        with torch.no_grad():
            for key, off, n in st["layout"]:
                p = params[key]
                if p.data_ptr() != base + 4 * off or p.dtype != torch.float32:
                    flat[off:off + n].copy_(p.detach().reshape(-1).to(device=device, dtype=torch.float32))
                    p.data = flat[off:off + n].view(p.shape)
        return flat

    # ---- flat-gradient mode (esc.optim.FlatAdamW) ----------------------------------------------------
    def enable_flat_grads(self, device):
        """Every p.grad becomes a view of ONE flat gradient buffer that the training backward fills directly (accumulating across
        backward calls until zero_flat_grads), so that the optimiser is two kernels over flat buffers.  autograd's per-parameter
        accumulation (and therefore per-parameter hooks such as DDP's) is bypassed in this mode."""
        device = torch.device(device)
        lib, hd = self._handle(device, for_training=True)
        flat = self._ensure_flat(device, lib, hd)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        st = self._flat[idx]
        if "gflat" not in st:
            old = self._carry.pop(idx, None)             # a rebuild (model.to(), load_state_dict) keeps pending gradients: same layout, same buffer
            if old is not None and old[0].shape == flat.shape and old[0].device == flat.device:
                st["gflat"], st["gfresh"] = old
            else:
                st["gflat"], st["gfresh"] = torch.zeros_like(flat), True
        params = self._named_params()
        for key, off, n in st["layout"]:
            params[key].grad = st["gflat"][off:off + n].view(params[key].shape)
        self._flat_grad_mode = True

    def flat_buffers(self, device):
        device = torch.device(device)
        lib, hd = self._handle(device, for_training=True)
        flat = self._ensure_flat(device, lib, hd)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if "gflat" not in self._flat[idx]:
            self.enable_flat_grads(device)
        return flat, self._flat[idx]["gflat"]

    def zero_flat_grads(self, device):
        idx = torch.device(device).index
        idx = idx if idx is not None else torch.cuda.current_device()
        st = self._flat.get(idx)
        if st is not None and "gflat" in st:
            st["gfresh"] = True                      # the next backward overwrites instead of accumulating: no memset needed

    def note_params_updated(self):
        """The flat buffer was written by a native kernel (no autograd version bump): mark every packed layout stale."""
        self._packed_version = {}

    def _handle(self, device: torch.device, for_training: bool = False):
        lib = _native.load()
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if self._dirty:
            for hd in self._handles.values():
                lib.escx_destroy(hd)
            # flat-gradient mode outlives the rebuild: the gradient buffer (and with it every p.grad view and whatever a backward has already
            # accumulated) is carried over, so that a live FlatAdamW keeps stepping on real gradients
            self._carry = {i: (st["gflat"], st["gfresh"]) for i, st in self._flat.items() if "gflat" in st}
            self._handles, self._flat, self._packed_version = {}, {}, {}
            self._dirty = False
        if idx not in self._handles:
            hd = ctypes.c_void_p()
            self._create_handle(lib, idx, hd)
            try:
                for key, t in self.state_dict().items():
                    if not t.is_floating_point():
                        continue
                    host = t.detach().to("cpu", torch.float32).contiguous()
                    shape = (ctypes.c_int64 * max(host.dim(), 1))(*host.shape)
                    _native.check(lib.escx_set_param(hd, key.encode(), host.data_ptr(), shape, host.dim()))
                _native.check(lib.escx_finalize_params(hd))
                if self._precision is not None:
                    _native.check(lib.escx_set_precision(hd, _native.PRECISIONS[self._precision]))
            except Exception:
                lib.escx_destroy(hd)
                raise
            self._handles[idx] = hd
            self._packed_version[idx] = self._param_version()
            if self._flat_grad_mode and idx in self._carry:
                self._flat_grad_mode = False             # (guards the re-entry through enable_flat_grads -> _handle)
                self.enable_flat_grads(device)
        hd = self._handles[idx]
        if not for_training and self._packed_version.get(idx) != self._param_version():
            # parameters were updated in place since the last pack (optimizer steps, manual edits): rebuild every derived layout,
            # including the host-folded ones of the inference path, from the current values
            flat = self._ensure_flat(device, lib, hd)
            with torch.cuda.device(device):
                _native.check(lib.escx_load_flat_params(hd, ctypes.c_void_p(flat.data_ptr()), 1, self._stream(device)))
            self._packed_version[idx] = self._param_version()
        return lib, hd

    def __getstate__(self):
        """copy.deepcopy / torch.save of the whole module: native handles are per-process device resources and are rebuilt lazily."""
        state = self.__dict__.copy()
        state["_handles"], state["_flat"], state["_packed_version"], state["_dirty"], state["_carry"] = {}, {}, {}, True, {}
        state["_flat_grad_mode"] = False
        return state

    def __del__(self):
        try:
            lib = _native.load()
            for hd in self._handles.values():
                lib.escx_destroy(hd)
        except Exception:
            pass

    @staticmethod
    def _need_gpu(t: torch.Tensor, what: str):
        if not t.is_cuda:
            raise RuntimeError(f"esc.ESC (MI355X build): {what} must live on a HIP device (got {t.device}); "
                               "this package has no CPU implementation of the encode/decode path")

    @staticmethod
    def _stream(device) -> ctypes.c_void_p:
        return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)

    def reserve(self, batch: int, n_samples: int, device=None):
        """Pre-size the workspace (otherwise done on first use; resizing synchronises the device)."""
        device = torch.device(device) if device is not None else next(self.parameters()).device
        lib, hd = self._handle(device)
        _native.check(lib.escx_reserve(hd, batch, n_samples))

    def latent_shape(self, n_samples: int) -> Tuple[int, int]:
        pf, pt = self.cfg["patch_size"]
        T = 1 + n_samples // self.hop_length
        H = self.in_freq // pf
        for _ in range(len(self.enc_h_dims) - 1):
            H = (H + 1) // 2
        return H, T // pt

    @staticmethod
    def _is_per_clip(num_streams) -> bool:
        """True for per-clip stream counts (a sequence or a 1-D tensor / array), False for one count for the whole batch."""
        if isinstance(num_streams, (str, bytes)):
            return False
        if isinstance(num_streams, torch.Tensor) or hasattr(num_streams, "ndim"):
            return int(num_streams.ndim) > 0
        return isinstance(num_streams, (list, tuple, range))

    def _per_clip_streams(self, num_streams, B: int) -> Optional[List[int]]:
        """None when `num_streams` is one count for the whole batch; else the per-clip counts (length B, each in [1, max_streams]; RVQCodecs: num_rvqs)."""
        if not self._is_per_clip(num_streams):
            return None
        if isinstance(num_streams, torch.Tensor):
            if num_streams.dim() != 1 or num_streams.dtype.is_floating_point or num_streams.dtype.is_complex or num_streams.dtype == torch.bool:
                raise ValueError(f"per-clip num_streams must be a 1-D integer tensor (got {num_streams.dtype}, {num_streams.dim()}-D)")
            vals = num_streams.tolist()
        else:
            if int(getattr(num_streams, "ndim", 1)) != 1:
                raise ValueError("per-clip num_streams must be one-dimensional")
            vals = list(num_streams)
        out = []
        for v in vals:
            if isinstance(v, bool) or isinstance(v, float):
                raise ValueError(f"per-clip num_streams must be integers (got {v!r})")
            try:
                out.append(operator.index(v))
            except TypeError:
                raise ValueError(f"per-clip num_streams must be integers (got {v!r})") from None
        if len(out) != B:
            raise ValueError(f"per-clip num_streams has {len(out)} entries for a batch of {B} clips")
        for b, v in enumerate(out):
            if not 1 <= v <= self._code_streams:
                raise ValueError(f"num_streams[{b}]={v} outside [1, {self._code_streams}]")
        return out

    # ---- mixed-length batches (include/escx.h escx_encode_lengths) ----------------------------------------
    _supports_lengths = True            # RVQCodecs: False

    def frame_lengths(self, lengths) -> List[int]:
        """Latent frames W_b of clips of `lengths` samples: latent_shape(L_b)[1]."""
        return [self.latent_shape(int(L))[1] for L in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]

    def output_lengths(self, frame_lengths) -> List[int]:
        """Samples decode returns for clips of `frame_lengths` latent frames: hop * (patch_t * W_b - 1)."""
        pt = self.cfg["patch_size"][1]
        return [self.hop_length * (pt * int(W) - 1) for W in (frame_lengths.tolist() if isinstance(frame_lengths, torch.Tensor) else frame_lengths)]

    def _check_lengths_call(self, what: str, num_streams=None, x_feat=None):
        """The refusals of a call with per-clip lengths (none of them needs a device)."""
        if not self._supports_lengths:
            raise NotImplementedError(f"{type(self).__name__}: {what} (mixed-length batches) is implemented for ESC (csvq+swinT) only, not for RVQCodecs")
        if self.cfg["window_size"] != 4:
            raise NotImplementedError(f"{what} (mixed-length batches) is implemented for window_size 4 only (this model: {self.cfg['window_size']})")
        if self.training:
            raise ValueError(f"{what} (mixed-length batches) is an inference feature: call model.eval() first; the training step takes equal-length clips")
        if num_streams is not None and self._is_per_clip(num_streams):
            raise NotImplementedError(f"{what} together with per-clip num_streams is not implemented: a mixed-length batch takes one num_streams")
        if x_feat is not None:
            raise NotImplementedError(f"{what} together with x_feat is not implemented: a mixed-length batch starts from the waveform")

    @staticmethod
    def _int_list(values, what: str, B: int) -> List[int]:
        """A sequence or 1-D integer tensor of B integers -> list; anything else is a ValueError."""
        if isinstance(values, (str, bytes)) or values is None:
            raise ValueError(f"{what} must be a sequence or a 1-D integer tensor of {B} values (got {values!r})")
        if isinstance(values, torch.Tensor):
            if values.dim() != 1 or values.dtype.is_floating_point or values.dtype.is_complex or values.dtype == torch.bool:
                raise ValueError(f"{what} must be a 1-D integer tensor (got {values.dtype}, {values.dim()}-D)")
            vals = values.tolist()
        else:
            if int(getattr(values, "ndim", 1)) != 1:
                raise ValueError(f"{what} must be one-dimensional")
            try:
                vals = list(values)
            except TypeError:
                raise ValueError(f"{what} must be a sequence or a 1-D integer tensor of {B} values (got {values!r})") from None
        out = []
        for v in vals:
            if isinstance(v, (bool, float)):
                raise ValueError(f"{what} must be integers (got {v!r})")
            try:
                out.append(operator.index(v))
            except TypeError:
                raise ValueError(f"{what} must be integers (got {v!r})") from None
        if len(out) != B:
            raise ValueError(f"{what} has {len(out)} entries for a batch of {B} clips")
        return out

    def _sample_lengths(self, lengths, B: int, Lx: int) -> Tuple[List[int], List[int]]:
        """Per-clip sample counts -> (lengths, latent widths); n_fft // 2 < L_b <= Lx, and every W_b a multiple of `overlap` (the single-clip call's assertion)."""
        vals = self._int_list(lengths, "lengths", B)
        half = self.in_freq - 1                         # n_fft // 2 with n_fft = 2 (in_freq - 1): the reflect padding of torch.stft(center=True)
        for b, L in enumerate(vals):
            if not half < L <= Lx:
                raise ValueError(f"lengths[{b}]={L} outside ({half}, {Lx}]: a clip is longer than the reflect padding and no longer than x.shape[1]")
        widths = [self.latent_shape(L)[1] for L in vals]
        for b, W in enumerate(widths):
            if W < 1 or W % self.cfg["overlap"] != 0:
                raise AssertionError(f"Time dimension must be multiple of overlap (clip {b}: {vals[b]} samples give {W} latent frames)")       # quantization.py:407
        return vals, widths

    # ---- public API (codecs.py:48-94) ---------------------------------------------------------
    @torch.no_grad()
    def encode(self, x: torch.Tensor, num_streams=6, lengths=None):
        """(Bs, L) waveform -> codes (Bs, num_streams, group_size, W/overlap) int64, feat_shape (H, W).
        `num_streams` may also be a length-Bs sequence or 1-D integer tensor of per-clip counts (a mixed-bitrate batch): the codes are then
        (Bs, max(num_streams), group_size, W/overlap) with -1 in the slots past each clip's own count, and clip b's codes equal those of
        encode(x[b:b+1], num_streams[b]).
        `lengths` (a length-Bs sequence or 1-D integer tensor of sample counts, n_fft // 2 < L_b <= L) makes the batch a mixed-length one: clip b is
        x[b, :L_b] (what is stored past it is not read) and gets the codes of encode(x[b:b+1, :L_b], num_streams); codes are
        (Bs, num_streams, group_size, Wmax/overlap) with Wmax = max(frame_lengths(lengths)) and -1 at the frames >= W_b/overlap, feat_shape (H, Wmax)."""
        if x.dim() != 2:
            raise ValueError("x must have shape (Bs, L)")
        if lengths is not None:
            return self._encode_lengths(x, num_streams, lengths)
        streams = self._per_clip_streams(num_streams, x.shape[0])
        self._need_gpu(x, "x")
        if streams is not None:
            return self._encode_streams(x, streams)
        x = x.to(torch.float32).contiguous()
        lib, hd = self._handle(x.device)
        B, L = x.shape
        _, W = self.latent_shape(L)
        if W % self.cfg["overlap"] != 0:
            raise AssertionError("Time dimension must be multiple of overlap")       # quantization.py:407
        codes = torch.empty((B, int(num_streams), self.cfg["group_size"], W // self.cfg["overlap"]), dtype=torch.int64,
                            device=x.device)
        if B == 0:                                      # empty batch: the reference returns empty codes and the latent shape
            return codes, self.latent_shape(L)
        fh, fw = ctypes.c_int(), ctypes.c_int()
        with torch.cuda.device(x.device):
            _native.check(lib.escx_encode(hd, x.data_ptr(), B, L, int(num_streams), codes.data_ptr(), ctypes.byref(fh),
                                          ctypes.byref(fw), self._stream(x.device)))
        return codes, (fh.value, fw.value)

    def _encode_lengths(self, x: torch.Tensor, num_streams, lengths):
        self._check_lengths_call("encode(lengths=...)", num_streams)
        B, Lx = x.shape
        vals, widths = self._sample_lengths(lengths, B, Lx)
        self._need_gpu(x, "x")
        x = x.to(torch.float32).contiguous()
        H = self.latent_shape(Lx)[0]
        Wmax = max(widths, default=0)
        codes = torch.empty((B, int(num_streams), self.cfg["group_size"], Wmax // self.cfg["overlap"]), dtype=torch.int64, device=x.device)
        if B == 0:
            return codes, (H, Wmax)
        lib, hd = self._handle(x.device)
        fh, fw = ctypes.c_int(), ctypes.c_int()
        with torch.cuda.device(x.device):
            _native.check(lib.escx_encode_lengths(hd, x.data_ptr(), B, Lx, (ctypes.c_int32 * B)(*vals), int(num_streams), codes.data_ptr(),
                                                  ctypes.byref(fh), ctypes.byref(fw), self._stream(x.device)))
        return codes, (fh.value, fw.value)

    def _encode_streams(self, x: torch.Tensor, streams: List[int]):
        x = x.to(torch.float32).contiguous()
        B, L = x.shape
        _, W = self.latent_shape(L)
        if W % self.cfg["overlap"] != 0:
            raise AssertionError("Time dimension must be multiple of overlap")       # quantization.py:407
        codes = torch.empty((B, max(streams, default=0), self.cfg["group_size"], W // self.cfg["overlap"]), dtype=torch.int64, device=x.device)
        if B == 0:
            return codes, self.latent_shape(L)
        lib, hd = self._handle(x.device)
        fh, fw = ctypes.c_int(), ctypes.c_int()
        counts = (ctypes.c_int32 * B)(*streams)
        with torch.cuda.device(x.device):
            _native.check(lib.escx_encode_streams(hd, x.data_ptr(), B, L, counts, codes.data_ptr(), ctypes.byref(fh), ctypes.byref(fw),
                                                  self._stream(x.device)))
        return codes, (fh.value, fw.value)

    @torch.no_grad()
    def decode(self, codes: torch.Tensor, feat_shape=(2, 1000), return_feat: bool = False, num_streams=None, frame_lengths=None):
        """codes (Bs, num_streams, group_size, *) + feat_shape (H, W) -> waveform (Bs, hop*(2W-1)).
        num_streams=None: every clip carries codes.size(1) streams.  A length-Bs sequence / 1-D integer tensor gives each clip its own
        count (at most codes.size(1)); the slots at or past it are never read.
        frame_lengths (a length-Bs sequence / 1-D integer tensor of latent widths W_b, multiples of `overlap`, at most W): a mixed-length batch - clip b
        is decoded from its own W_b/overlap code frames (the others are never read) as decode(codes[b:b+1, :, :, :W_b/overlap], (H, W_b)) would; its
        audio is exactly 0 from output_lengths(frame_lengths)[b] on, and the spectrum of return_feat=True is zero past patch_t * W_b frames."""
        if codes.dim() != 4:
            raise ValueError("codes must have shape (Bs, num_streams, group_size, T)")
        if frame_lengths is not None:
            return self._decode_lengths(codes, feat_shape, return_feat, num_streams, frame_lengths)
        streams = None
        if num_streams is not None:
            if not self._is_per_clip(num_streams):
                raise ValueError("decode(num_streams=...) takes per-clip counts (a sequence or 1-D tensor); a uniform count is codes.size(1)")
            streams = self._per_clip_streams(num_streams, codes.shape[0])
            if streams and max(streams) > codes.shape[1]:
                raise ValueError(f"num_streams up to {max(streams)} but codes carry {codes.shape[1]} stream slots")
        self._need_gpu(codes, "codes")
        codes = codes.to(torch.int64).contiguous()
        lib, hd = self._handle(codes.device)
        B, S, G, Tq = codes.shape
        H, W = int(feat_shape[0]), int(feat_shape[1])
        if G != self.cfg["group_size"] or Tq * self.cfg["overlap"] != W:
            raise ValueError(f"codes shape {tuple(codes.shape)} does not match feat_shape {(H, W)}")
        pt = self.cfg["patch_size"][1]
        out = torch.empty((B, self.hop_length * (pt * W - 1)), dtype=torch.float32, device=codes.device)
        feat = torch.empty((B, pt * W, self.in_dim, self.in_freq), dtype=torch.float32, device=codes.device) if return_feat else None
        if B == 0:
            return (out, feat.permute(0, 2, 3, 1)) if return_feat else out
        with torch.cuda.device(codes.device):
            if streams is None:
                _native.check(lib.escx_decode(hd, codes.data_ptr(), B, S, H, W, out.data_ptr(),
                                              feat.data_ptr() if return_feat else None, self._stream(codes.device)))
            else:
                _native.check(lib.escx_decode_streams(hd, codes.data_ptr(), B, S, (ctypes.c_int32 * B)(*streams), H, W, out.data_ptr(),
                                                      feat.data_ptr() if return_feat else None, self._stream(codes.device)))
        if return_feat:
            return out, feat.permute(0, 2, 3, 1)
        return out

    def _decode_lengths(self, codes, feat_shape, return_feat, num_streams, frame_lengths):
        self._check_lengths_call("decode(frame_lengths=...)", num_streams)
        if num_streams is not None:
            raise ValueError("decode(num_streams=...) takes per-clip counts (a sequence or 1-D tensor); a uniform count is codes.size(1)")
        B, S, G, Tq = codes.shape
        H, W = int(feat_shape[0]), int(feat_shape[1])
        ov, pt = self.cfg["overlap"], self.cfg["patch_size"][1]
        if G != self.cfg["group_size"] or Tq * ov != W:
            raise ValueError(f"codes shape {tuple(codes.shape)} does not match feat_shape {(H, W)}")
        widths = self._int_list(frame_lengths, "frame_lengths", B)
        for b, Wb in enumerate(widths):
            if not 1 <= Wb <= W:
                raise ValueError(f"frame_lengths[{b}]={Wb} outside [1, {W}] (feat_shape[1])")
            if Wb % ov != 0:
                raise AssertionError(f"Time dimension must be multiple of overlap (clip {b}: {Wb} latent frames)")
        self._need_gpu(codes, "codes")
        codes = codes.to(torch.int64).contiguous()
        out = torch.empty((B, self.hop_length * (pt * W - 1)), dtype=torch.float32, device=codes.device)
        feat = torch.empty((B, pt * W, self.in_dim, self.in_freq), dtype=torch.float32, device=codes.device) if return_feat else None
        if B > 0:
            lib, hd = self._handle(codes.device)
            with torch.cuda.device(codes.device):
                _native.check(lib.escx_decode_lengths(hd, codes.data_ptr(), B, S, (ctypes.c_int32 * B)(*widths), H, W, out.data_ptr(),
                                                      feat.data_ptr() if return_feat else None, self._stream(codes.device)))
        return (out, feat.permute(0, 2, 3, 1)) if return_feat else out

    def _forward_lengths(self, x, x_feat, num_streams, lengths):
        """Eval forward of a mixed-length batch (escx_forward_lengths): the composition of encode(lengths=...) and decode(frame_lengths=...).  raw_feat is
        (Bs, 2, F, Tmax) with Tmax = 1 + max(lengths) // hop and zeros past a clip's own frames; cm_loss / cb_loss are means over a clip's own frames."""
        self._check_lengths_call("forward(lengths=...)", num_streams, x_feat)
        if x.dim() != 2:
            raise ValueError("x must have shape (Bs, L)")
        B, Lx = x.shape
        vals, widths = self._sample_lengths(lengths, B, Lx)
        self._need_gpu(x, "x")
        xin = x.to(torch.float32).contiguous()
        dev = xin.device
        S, pt, ov = int(num_streams), self.cfg["patch_size"][1], self.cfg["overlap"]
        Wmax = max(widths, default=0)
        T = 1 + max(vals, default=0) // self.hop_length
        codes = torch.empty((B, S, self.cfg["group_size"], Wmax // ov), dtype=torch.int64, device=dev)
        recon = torch.empty((B, max(self.hop_length * (pt * Wmax - 1), 0)), dtype=torch.float32, device=dev)
        raw_feat = torch.empty((B, T, self.in_dim, self.in_freq), dtype=torch.float32, device=dev)
        recon_feat = torch.empty((B, pt * Wmax, self.in_dim, self.in_freq), dtype=torch.float32, device=dev)
        cm = torch.empty((B,), dtype=torch.float32, device=dev)
        if B > 0:
            lib, hd = self._handle(dev)
            with torch.cuda.device(dev):
                _native.check(lib.escx_forward_lengths(hd, xin.data_ptr(), B, Lx, (ctypes.c_int32 * B)(*vals), S, codes.data_ptr(), recon.data_ptr(),
                                                       raw_feat.data_ptr(), recon_feat.data_ptr(), cm.data_ptr(), self._stream(dev)))
        return {"cm_loss": cm, "cb_loss": cm.clone(), "raw_audio": x, "recon_audio": recon,
                "raw_feat": raw_feat.permute(0, 2, 3, 1), "recon_feat": recon_feat.permute(0, 2, 3, 1), "codes": codes}

    def forward_one_step(self, x, x_feat=None, num_streams=6, freeze_codebook=False, lengths=None):
        if not self.training and freeze_codebook:
            raise ValueError("``freeze_vq`` must be set False during inference")       # quantization.py:43-44
        if lengths is not None:
            return self._forward_lengths(x, x_feat, num_streams, lengths)
        if self.training:
            if self._is_per_clip(num_streams):
                raise ValueError("per-clip num_streams is an inference feature: the training step draws one num_streams per batch "
                                 "(scripts/utils.py:11-25)")
            return self._forward_train(x, x_feat, int(num_streams), bool(freeze_codebook))
        if x_feat is not None:
            streams = self._per_clip_streams(num_streams, x_feat.shape[0]) if x_feat.dim() == 4 else None
            return self._forward_from_feat(x, x_feat, int(num_streams) if streams is None else streams)
        if x.dim() != 2:
            raise ValueError("x must have shape (Bs, L)")
        streams = self._per_clip_streams(num_streams, x.shape[0])
        self._need_gpu(x, "x")
        xin = x.to(torch.float32).contiguous()
        lib, hd = self._handle(xin.device)
        B, L = xin.shape
        S = int(num_streams) if streams is None else max(streams, default=0)
        _, W = self.latent_shape(L)
        if W % self.cfg["overlap"] != 0:
            raise AssertionError("Time dimension must be multiple of overlap")
        pt = self.cfg["patch_size"][1]
        T = 1 + L // self.hop_length
        dev = xin.device
        codes = torch.empty((B, S, self.cfg["group_size"], W // self.cfg["overlap"]), dtype=torch.int64, device=dev)
        recon = torch.empty((B, self.hop_length * (pt * W - 1)), dtype=torch.float32, device=dev)
        raw_feat = torch.empty((B, T, self.in_dim, self.in_freq), dtype=torch.float32, device=dev)
        recon_feat = torch.empty((B, pt * W, self.in_dim, self.in_freq), dtype=torch.float32, device=dev)
        cm = torch.empty((B,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            if B > 0 and streams is None:               # an empty batch returns the (empty) buffers as they are
                _native.check(lib.escx_forward(hd, xin.data_ptr(), B, L, S, codes.data_ptr(), recon.data_ptr(), raw_feat.data_ptr(),
                                               recon_feat.data_ptr(), cm.data_ptr(), self._stream(dev)))
            elif B > 0:                                 # per-clip counts: codes (B, max S, G, T), -1 past each clip's streams
                _native.check(lib.escx_forward_streams(hd, xin.data_ptr(), None, B, L, (ctypes.c_int32 * B)(*streams), codes.data_ptr(),
                                                       recon.data_ptr(), raw_feat.data_ptr(), recon_feat.data_ptr(), cm.data_ptr(), self._stream(dev)))
        return {"cm_loss": cm, "cb_loss": cm.clone(), "raw_audio": x, "recon_audio": recon,
                "raw_feat": raw_feat.permute(0, 2, 3, 1), "recon_feat": recon_feat.permute(0, 2, 3, 1), "codes": codes}

    def _forward_from_feat(self, x, x_feat, S):
        """forward(x, x_feat=...) of the reference (codecs.py:33-34): x_feat is the complex STFT as a real tensor laid out
        (Bs, F, T, 2) - what `rearrange(x_feat, "b h w c -> b c h w")` expects, despite the docstring - and replaces
        spec_transform(x).  The permutation to the library's frame-major layout is plain data movement.  S: one count, or a
        list of per-clip counts."""
        if x_feat.dim() != 4 or x_feat.shape[1] != self.in_freq or x_feat.shape[3] != self.in_dim:
            raise ValueError(f"x_feat must have shape (Bs, {self.in_freq}, T, {self.in_dim})")
        self._need_gpu(x_feat, "x_feat")
        feat = x_feat.to(torch.float32).permute(0, 2, 3, 1).contiguous()            # (B, T, 2, F)
        B, T = feat.shape[0], feat.shape[1]
        pt = self.cfg["patch_size"][1]
        W = T // pt
        if W < 1 or W % self.cfg["overlap"] != 0:
            raise AssertionError("Time dimension must be multiple of overlap")
        dev = feat.device
        lib, hd = self._handle(dev)
        streams = S if isinstance(S, list) else None
        Smax = max(streams, default=0) if streams is not None else S
        codes = torch.empty((B, Smax, self.cfg["group_size"], W // self.cfg["overlap"]), dtype=torch.int64, device=dev)
        recon = torch.empty((B, self.hop_length * (pt * W - 1)), dtype=torch.float32, device=dev)
        recon_feat = torch.empty((B, pt * W, self.in_dim, self.in_freq), dtype=torch.float32, device=dev)
        cm = torch.empty((B,), dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            if streams is None:
                _native.check(lib.escx_forward_feat(hd, feat.data_ptr(), B, T, S, codes.data_ptr(), recon.data_ptr(), recon_feat.data_ptr(),
                                                    cm.data_ptr(), self._stream(dev)))
            elif B > 0:
                _native.check(lib.escx_forward_streams(hd, None, feat.data_ptr(), B, T, (ctypes.c_int32 * B)(*streams), codes.data_ptr(),
                                                       recon.data_ptr(), None, recon_feat.data_ptr(), cm.data_ptr(), self._stream(dev)))
        return {"cm_loss": cm, "cb_loss": cm.clone(), "raw_audio": x, "recon_audio": recon,
                "raw_feat": x_feat.permute(0, 3, 1, 2), "recon_feat": recon_feat.permute(0, 2, 3, 1), "codes": codes}

    def _forward_train(self, x, x_feat, S, freeze):
        """Training-mode forward (codecs.py:30-46 with csrvq.py:97-129, codebook.py:57-75, quantization.py:53-64): differentiable w.r.t.
        every parameter and w.r.t. the input (x, or x_feat when given) through `_TrainStep`; `codes` holds all max_streams streams (every
        quantiser runs in training mode).  raw_feat is differentiable exactly when the input requires grad, as spec_transform(x) is in the reference."""
        if x.dim() != 2:
            raise ValueError("x must have shape (Bs, L)")
        if x_feat is not None and (x_feat.dim() != 4 or x_feat.shape[1] != self.in_freq or x_feat.shape[3] != self.in_dim or x_feat.shape[0] != x.shape[0]):
            raise ValueError(f"x_feat must have shape (Bs, {self.in_freq}, T, {self.in_dim})")
        self._need_gpu(x, "x")
        feat = None
        if x_feat is not None:          # codecs.py:33-34: the given spectrum replaces the STFT of x; layout (Bs, F, T, 2) as in eval mode (_forward_from_feat)
            self._need_gpu(x_feat, "x_feat")
            feat = x_feat.to(torch.float32).permute(0, 2, 3, 1).contiguous()      # frame-major (Bs, T, 2, F): the library's spectrum layout (differentiable)
        params = tuple(self.parameters())
        recon, recon_fm, raw_fm, cm, cb, codes = _TrainStep.apply(self, x.to(torch.float32).contiguous(), feat, S, freeze, *params)
        return {"cm_loss": cm, "cb_loss": cb, "raw_audio": x, "recon_audio": recon,
                "raw_feat": raw_fm.permute(0, 2, 3, 1), "recon_feat": recon_fm.permute(0, 2, 3, 1), "codes": codes}

    def forward(self, x, x_feat, num_streams, freeze_codebook=False, lengths=None):
        """codecs.py:48-66: dict with cm_loss, cb_loss, raw_audio, recon_audio, raw_feat (Bs,2,F,T), recon_feat (Bs,2,F,T'), codes.
        Eval mode: inference path, no autograd graph.  Training mode: differentiable (HIP forward + hand-written HIP backward).
        lengths (eval mode only): per-clip sample counts of a mixed-length batch, as in encode; see _forward_lengths."""
        num_streams = self.max_streams if freeze_codebook else num_streams
        if lengths is not None:
            with torch.no_grad():
                return self.forward_one_step(x, x_feat, num_streams, freeze_codebook, lengths)
        if self.training:
            return self.forward_one_step(x, x_feat, num_streams, freeze_codebook)
        with torch.no_grad():
            return self.forward_one_step(x, x_feat, num_streams, freeze_codebook)


class _TrainStep(torch.autograd.Function):
    """One training-mode pass through libescx: forward keeps its activations on the handle's tape, backward consumes them and returns
    d loss / d parameter for every nn.Parameter (views of one flat gradient buffer, the library's canonical order) and, when the input requires
    grad, d loss / d input (x, or the spectrum `feat` when given; the gradient of raw_feat is folded in).  With no parameter requiring grad the
    library is asked for the input gradient only (grad_flat = NULL): no p.grad is written and the flat-gradient buffers stay untouched."""

    @staticmethod
    def forward(ctx, model, x, feat, S, freeze, *params):
        dev = x.device
        lib, hd = model._handle(dev, for_training=True)
        flat = model._ensure_flat(dev, lib, hd)
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        model._packed_version[idx] = None               # the training refresh skips the host-folded inference layouts
        c = model.cfg
        B, L = x.shape
        if feat is not None:            # the spectrum decides the geometry (codecs.py:33-34): T frames <-> hop * (T - 1) samples
            L = model.hop_length * (feat.shape[1] - 1)
        _, W = model.latent_shape(L)
        if W % c["overlap"] != 0:
            raise AssertionError("Time dimension must be multiple of overlap")       # quantization.py:407
        pt = c["patch_size"][1]
        T = 1 + L // model.hop_length
        codes = torch.empty((B, model._code_streams, c["group_size"], W // c["overlap"]), dtype=torch.int64, device=dev)      # every quantiser runs in training mode
        recon = torch.empty((B, model.hop_length * (pt * W - 1)), dtype=torch.float32, device=dev)
        raw_fm = feat if feat is not None else torch.empty((B, T, model.in_dim, model.in_freq), dtype=torch.float32, device=dev)
        recon_fm = torch.empty((B, pt * W, model.in_dim, model.in_freq), dtype=torch.float32, device=dev)
        cm = torch.empty((B,), dtype=torch.float32, device=dev)
        cb = torch.empty((B,), dtype=torch.float32, device=dev)
        P = lambda t: ctypes.c_void_p(t.data_ptr())
        with torch.cuda.device(dev):
            _native.check(model._train_forward_call(lib, hd, P(flat), P(x), P(feat) if feat is not None else None, B, T if feat is not None else L, int(S), int(bool(freeze)),
                                                    P(codes), P(recon), P(raw_fm), P(recon_fm), P(cm), P(cb), model._stream(dev)))
        ctx.model, ctx.dev, ctx.idx = model, dev, idx
        ctx.tape_generation = int(lib.escx_train_tape_generation(hd))
        ctx.from_feat = feat is not None
        ctx.in_shape = tuple(feat.shape) if feat is not None else (B, L)
        ctx.input_grad = bool(ctx.needs_input_grad[2] if feat is not None else ctx.needs_input_grad[1])
        if ctx.input_grad:              # raw_feat = spec_transform(x) (or x_feat itself) is differentiable in the reference
            ctx.mark_non_differentiable(codes)
        else:
            ctx.mark_non_differentiable(raw_fm, codes)
        return recon, recon_fm, raw_fm, cm, cb, codes

    @staticmethod
    def backward(ctx, d_recon, d_recon_fm, d_raw, d_cm, d_cb, _d_codes):
        model, dev = ctx.model, ctx.dev
        n_params = len(ctx.needs_input_grad) - 5
        want_params = any(ctx.needs_input_grad[5:])
        if not want_params and not ctx.input_grad:
            return (None,) * (5 + n_params)
        lib, hd = model._handle(dev, for_training=True)
        if int(lib.escx_train_tape_generation(hd)) != ctx.tape_generation:
            raise RuntimeError("esc.ESC backward: the model ran another training forward after the one this graph belongs to; the library keeps ONE "
                               "activation tape per model (backward before the next forward, or use a second model instance)")
        if ctx.input_grad:
            return _TrainStep._backward_with_input(ctx, lib, hd, want_params, d_recon, d_recon_fm, d_raw, d_cm, d_cb)
        st = model._flat[ctx.idx]
        flat_mode = model._flat_grad_mode and "gflat" in st
        gflat = st["gflat"] if (flat_mode and st["gfresh"]) else torch.empty_like(st["flat"])

        def prep(t):
            return None if t is None else t.to(torch.float32).contiguous()
        d_recon, d_recon_fm, d_cm, d_cb = prep(d_recon), prep(d_recon_fm), prep(d_cm), prep(d_cb)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(dev):
            _native.check(model._train_backward_call(lib, hd, p(d_recon), p(d_recon_fm), None, p(d_cm), p(d_cb), p(gflat), None, False, model._stream(dev)))
        params = model._named_params()
        if flat_mode:                                   # p.grad are views of st["gflat"]: written in place, nothing for autograd to accumulate
            if st["gfresh"]:
                st["gfresh"] = False
            else:
                st["gflat"].add_(gflat)
            return (None, None, None, None, None) + (None,) * len(params)
        by_id = {id(params[k]): gflat[off:off + n].view(params[k].shape) for k, off, n in st["layout"]}
        grads = tuple(by_id.get(id(q)) for q in model.parameters())
        return (None, None, None, None, None) + grads

    @staticmethod
    def _backward_with_input(ctx, lib, hd, want_params, d_recon, d_recon_fm, d_raw, d_cm, d_cb):
        """escx_train_backward_ex (RVQCodecs: escx_rvq_train_backward): the input gradient, with the parameter gradients of `backward` when any parameter requires grad."""
        model, dev = ctx.model, ctx.dev
        n_params = len(ctx.needs_input_grad) - 5
        st = model._flat[ctx.idx]
        flat_mode = model._flat_grad_mode and "gflat" in st
        gflat = None
        if want_params:
            gflat = st["gflat"] if (flat_mode and st["gfresh"]) else torch.empty_like(st["flat"])

        def prep(t):
            return None if t is None else t.to(torch.float32).contiguous()
        d_recon, d_recon_fm, d_raw, d_cm, d_cb = prep(d_recon), prep(d_recon_fm), prep(d_raw), prep(d_cm), prep(d_cb)
        d_in = torch.empty(ctx.in_shape, dtype=torch.float32, device=dev)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        with torch.cuda.device(dev):
            _native.check(model._train_backward_call(lib, hd, p(d_recon), p(d_recon_fm), p(d_raw), p(d_cm), p(d_cb), p(gflat), p(d_in), True, model._stream(dev)))
        head = (None, None, d_in, None, None) if ctx.from_feat else (None, d_in, None, None, None)
        if not want_params:
            return head + (None,) * n_params
        params = model._named_params()
        if flat_mode:
            if st["gfresh"]:
                st["gfresh"] = False
            else:
                st["gflat"].add_(gflat)
            return head + (None,) * n_params
        by_id = {id(params[k]): gflat[off:off + n].view(params[k].shape) for k, off, n in st["layout"]}
        return head + tuple(by_id.get(id(q)) for q in model.parameters())


class RVQCodecs(ESC):
    """The rvq+swinT ablation codec (codecs.py:96-181): ESC's Swin encoder and decoder with plain product-residual VQ at the bottleneck
    (quantization.py:292-431) in place of the cross-scale quantisers, MI355X-native execution (fused_prvq.h: one HIP launch per batch part for
    the whole quantiser; train_prvq.h: its training form and backward).  encode, decode and the eval-mode forward take per-clip num_streams as in ESC; the
    training-mode forward is ESC's step (`_TrainStep`: HIP forward, hand-written HIP backward, input gradient, flat gradients) with the one bottleneck quantiser."""

    def __init__(self, in_dim: int = 2, in_freq: int = 192, h_dims: list = [45, 72, 96, 144, 192, 384], max_streams: int = 6,
                 backbone: Literal['transformer', 'convolution'] = 'transformer', kernel_size: list = [5, 2], conv_depth: int = 1,
                 patch_size: list = [3, 2], swin_heads: list = [3, 6, 12, 24, 24], swin_depth: int = 2, window_size: int = 4,
                 mlp_ratio: float = 4., overlap: int = 2, num_rvqs: int = 6, group_size: int = 3, codebook_dim: int = 8,
                 codebook_size: int = 1024, l2norm: bool = True, win_len: int = 20, hop_len: int = 5, sr: int = 16000) -> None:
        if backbone != "transformer":
            raise NotImplementedError("only backbone='transformer' (rvq+swinT) is implemented; the convolution "
                                      "backbone is an ablation outside the accelerated path")
        if int(num_rvqs) < 1:
            raise ValueError(f"num_rvqs={num_rvqs}: at least one residual stage")
        object.__setattr__(self, "_rvq", dict(num_rvqs=int(num_rvqs), codebook_dim=int(codebook_dim)))     # read by _state_manifest during ESC.__init__
        super().__init__(in_dim=in_dim, in_freq=in_freq, h_dims=h_dims, max_streams=max_streams, win_len=win_len, hop_len=hop_len, sr=sr,
                         patch_size=patch_size, swin_heads=swin_heads, swin_depth=swin_depth, window_size=window_size, mlp_ratio=mlp_ratio,
                         overlap=overlap, group_size=group_size, codebook_size=codebook_size, codebook_dims=[codebook_dim] * max_streams,
                         l2norm=l2norm, backbone=backbone, kernel_size=kernel_size, conv_depth=conv_depth)
        self.cfg.update(self._rvq)
        self.num_rvqs, self.codebook_dim = self._rvq["num_rvqs"], self._rvq["codebook_dim"]
        # max_bps: base.py:81 is ESC's expression (base.py:70) with num_product_vqs = group_size, set by ESC.__init__

    def _state_manifest(self) -> Dict[str, Tuple[int, ...]]:
        return rvq_state_manifest(dict(self.cfg, **self._rvq))

    @property
    def _code_streams(self) -> int:
        return self._rvq["num_rvqs"]

    _supports_lengths = False           # mixed-length batches: ESC only

    def _create_handle(self, lib, idx: int, hd: ctypes.c_void_p):
        rc = _native.EscxRvqConfig()
        rc.base = self._c_config()
        rc.num_rvqs, rc.codebook_dim = self._rvq["num_rvqs"], self._rvq["codebook_dim"]
        _native.check(lib.escx_create_rvq(ctypes.byref(rc), idx, ctypes.byref(hd)))

    def _train_forward_call(self, lib, hd, flat, x, feat, B, n, S, freeze, codes, recon, raw_fm, recon_fm, cm, cb, stream):
        return lib.escx_rvq_train_forward(hd, flat, x if feat is None else None, feat, B, n, S, freeze, codes, recon, raw_fm if feat is None else None, recon_fm, cm, cb, stream)

    def _train_backward_call(self, lib, hd, d_recon, d_recon_fm, d_raw, d_cm, d_cb, gflat, d_in, with_input, stream):
        return lib.escx_rvq_train_backward(hd, d_recon, d_recon_fm, d_raw, d_cm, d_cb, gflat, d_in, stream)

    def _streams_arg(self, num_streams):
        """An integer count above num_rvqs gives num_rvqs streams, as the reference's quantize_to_code loop does (quantization.py:230-243);
        a count below 1 is refused.  Per-clip sequences pass through (ESC's checks, bounded by num_rvqs)."""
        if self._is_per_clip(num_streams):
            return num_streams
        try:
            S = operator.index(num_streams)
        except TypeError:
            raise ValueError(f"num_streams must be an integer (got {num_streams!r})") from None
        if S < 1:
            raise ValueError(f"num_streams={S}: at least one residual stage")
        return min(S, self._rvq["num_rvqs"])

    @torch.no_grad()
    def encode(self, x: torch.Tensor, num_streams=6, lengths=None):
        """(Bs, L) waveform -> codes (Bs, min(num_streams, num_rvqs), group_size, W/overlap) int64, feat_shape (H, W) (codecs.py:166-171).
        Per-clip counts as in ESC.encode (each in [1, num_rvqs]).  lengths: NotImplementedError (mixed-length batches are ESC's)."""
        if lengths is not None:
            self._check_lengths_call("encode(lengths=...)")
        return super().encode(x, self._streams_arg(num_streams))

    def forward(self, x, x_feat, num_streams, freeze_codebook=False, lengths=None):
        """codecs.py:127-167.  Eval mode: the ESC dict, codes (Bs, min(num_streams, num_rvqs), group_size, T),
        cm_loss = cb_loss = sum over groups and stages of mse(z_q_i, residual_i).mean([1, 2]) / group_size.
        Training mode (on a HIP device): differentiable like ESC's; every stage runs, so codes is (Bs, num_rvqs, group_size, T), and the stages
        >= num_streams are masked out of the reconstruction and the losses (quantization.py:185-187); freeze_codebook as quantization.py:319-321."""
        if lengths is not None:
            self._check_lengths_call("forward(lengths=...)")
        if self.training:
            S = self._streams_arg(num_streams)
            if self._is_per_clip(S):
                raise ValueError("per-clip num_streams is an inference feature: the training step draws one num_streams per batch "
                                 "(scripts/utils.py:11-25)")
            t = next((v for v in (x, x_feat) if v is not None and not (isinstance(v, torch.Tensor) and v.is_cuda)), None)
            if t is not None:
                raise NotImplementedError("RVQCodecs training is not implemented for CPU tensors: the training step runs on a HIP device only "
                                          f"(got {getattr(t, 'device', type(t).__name__)}); this package has no CPU implementation of anything")
            return self.forward_one_step(x, x_feat, S, bool(freeze_codebook))
        if freeze_codebook:
            raise NotImplementedError("RVQCodecs: freeze_codebook is a training option (quantization.py:326-328); not implemented")
        with torch.no_grad():
            return self.forward_one_step(x, x_feat, self._streams_arg(num_streams), False)


model_dict = {"csvq+swinT": ESC, "rvq+swinT": RVQCodecs}


# kwargs an rvq+swinT configuration must state for make_model: the quantiser that distinguishes the ablation from ESC
# (configs/ablations/9kbps_rvq_swinT.yaml names both)
_RVQ_REQUIRED = ("num_rvqs", "codebook_dim")


def make_model(model_config, model_name: str = "csvq+swinT"):
    """codecs.py:190-200.  `model_name` defaults to the ESC codec so that scripts/compress.py:22 (which passes only the
    config) works.  "rvq+swinT" is built from a configuration that states its bottleneck quantiser (num_rvqs, codebook_dim, as
    the ablation yaml does); a configuration without them raises NotImplementedError - RVQCodecs() itself keeps the reference's
    defaults."""
    if model_name not in model_dict:
        raise NotImplementedError(f"{model_name} is not available in the MI355X build (csvq+swinT and rvq+swinT); "
                                  "the *+conv models are ablations outside the accelerated path")
    m = model_dict[model_name]
    cfg = dict(model_config) if isinstance(model_config, dict) else dict(vars(model_config))
    if m is RVQCodecs:
        missing = [k for k in _RVQ_REQUIRED if k not in cfg]
        if missing:
            raise NotImplementedError(f"make_model(..., {model_name!r}) builds the rvq ablation from its configuration, which must state "
                                      f"{', '.join(missing)} (configs/ablations/9kbps_rvq_swinT.yaml); construct RVQCodecs() for the "
                                      "reference's defaults")
    return m(**cfg)
