"""The DAC baseline codec (Descript audio codec; reference baselines/descript/dac/model/dac.py:148-266, nn/quantize.py) on the MI355X.

Same constructor keywords, same state_dict keys and shapes (`*.weight_g`, `*.weight_v`, `*.bias`, `*.alpha`,
`quantizer.quantizers.{i}.codebook.weight`: reference checkpoints load with `load_state_dict(strict=True)`), same eval-mode
`encode` / `decode` / `forward` / `quantizer.from_codes`.  Every convolution, the weight normalisation and the residual quantiser run in
libescx (csrc/dac.hip); there is no PyTorch/CPU implementation here.  Inference only: training mode raises NotImplementedError.  The
frozen codec can sit inside a larger autograd graph (eval mode, padding on, input gradients only): `decode(z)` is differentiable in `z`
(`_DecodeGrad`), `encode(x)` in `x` through the encoder and the straight-through quantiser (`_EncodeGrad`), and `forward(x)` chains the two.
Fine-tuning (still eval mode): `set_trainable("decoder")` gives `decode` the decoder's parameter gradients (`_DecodeParamGrad`),
`set_encode_trainable("encoder" | "quantizer" | "both")` gives `encode` the encoder's and the quantiser's (`_EncodeParamGrad`), and with both
`forward(x)` delivers the gradient of every parameter of the model.

The quantiser is callable on its own, as the reference's public `model.quantizer` is: `quantizer(z, n_quantizers)` (quantize.py:127-198)
snaps a latent the caller brings to the codebooks, with the straight-through gradient in `z` (`_QuantizeGrad`) and, after
set_encode_trainable("quantizer" | "both"), the quantiser's parameter gradients (`_QuantizeParamGrad`); `quantizer.from_latents(latents)`
(quantize.py:222-255) searches every codebook independently on per-codebook latents and has no gradient.

Mixed-length batches (not part of the reference's surface): `encode` / `forward` take `lengths`, `decode` / `quantizer.from_codes` take
`frame_lengths`, one entry per clip; every clip's results are bitwise those of the call on that clip alone.

`DACFile`, `DAC.padding`, `DAC.compress` and `DAC.decompress` are CodecMixin's (reference baselines/descript/dac/model/base.py:15-294): files of any
length in overlapping windows on padding-free convolutions, all windows of a file as one batch.
"""
from __future__ import annotations

import ctypes
import functools
import math
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Sequence, Union

import numpy as np
import torch
import torch.nn as nn

from .. import _native
from ..models.codecs import _attach

_ENCODE_PARTS = {"encoder": 1, "quantizer": 2, "both": 3}       # set_encode_trainable -> escx_dac_encode_backward_params' `parts`


def _param_specs(enc_dim, enc_rates, latent, dec_dim, dec_rates, n_cb, cb_size, cb_dim):
    """(key, shape) of every parameter in the reference's named_parameters() order."""
    out = []

    def conv(p, cin, cout, k, transposed=False):
        out.extend([(p + "bias", (cout,)), (p + "weight_g", (cin, 1, 1) if transposed else (cout, 1, 1)),
                    (p + "weight_v", (cin, cout, k) if transposed else (cout, cin, k))])

    def snake(p, c):
        out.append((p + "alpha", (1, c, 1)))

    def res(p, c):
        snake(p + "block.0.", c); conv(p + "block.1.", c, c, 7); snake(p + "block.2.", c); conv(p + "block.3.", c, c, 1)

    c = enc_dim
    conv("encoder.block.0.", 1, c, 7)
    for i, s in enumerate(enc_rates):
        p = f"encoder.block.{i + 1}.block."
        for j in range(3):
            res(f"{p}{j}.", c)
        snake(f"{p}3.", c); conv(f"{p}4.", c, 2 * c, 2 * s)
        c *= 2
    snake(f"encoder.block.{len(enc_rates) + 1}.", c); conv(f"encoder.block.{len(enc_rates) + 2}.", c, latent, 3)
    for i in range(n_cb):
        p = f"quantizer.quantizers.{i}."
        conv(p + "in_proj.", latent, cb_dim, 1); conv(p + "out_proj.", cb_dim, latent, 1)
        out.append((p + "codebook.weight", (cb_size, cb_dim)))
    c = dec_dim
    conv("decoder.model.0.", latent, c, 7)
    for i, s in enumerate(dec_rates):
        p = f"decoder.model.{i + 1}.block."
        snake(p + "0.", c); conv(p + "1.", c, c // 2, 2 * s, transposed=True)
        for j in range(3):
            res(f"{p}{j + 2}.", c // 2)
        c //= 2
    snake(f"decoder.model.{len(dec_rates) + 1}.", c); conv(f"decoder.model.{len(dec_rates) + 2}.", c, 1, 7)
    return out


SUPPORTED_VERSIONS = ["1.0.0"]
_MAP_LIMIT = (1 << 32) - 64          # a feature map of one pass stays below 2^32 elements (csrc/dac.hip), rounded up to 64 floats


@dataclass
class DACFile:
    """The reference's container of a compressed signal (base.py:15-54), same fields and same on-disk layout: `np.save` of
    {"codes": uint16 (rows, n_codebooks, frames), "metadata": {input_db, original_length, sample_rate, chunk_length, channels, padding,
    dac_version}}.  rows = batch * channels.  `input_db` is carried as given (a float, a tensor or None): this port measures no loudness."""
    codes: torch.Tensor
    chunk_length: int
    original_length: int
    input_db: object
    channels: int
    sample_rate: int
    padding: bool
    dac_version: str

    def save(self, path):
        db = self.input_db
        if isinstance(db, torch.Tensor):
            db = db.detach().cpu().numpy()
        if db is not None:
            db = np.asarray(db, dtype=np.float32)
        artifacts = {"codes": self.codes.detach().cpu().numpy().astype(np.uint16),
                     "metadata": {"input_db": db, "original_length": int(self.original_length), "sample_rate": int(self.sample_rate),
                                  "chunk_length": int(self.chunk_length), "channels": int(self.channels), "padding": bool(self.padding),
                                  "dac_version": SUPPORTED_VERSIONS[-1]}}
        path = Path(path).with_suffix(".dac")
        with open(path, "wb") as f:
            np.save(f, artifacts)
        return path

    @classmethod
    def load(cls, path):
        artifacts = np.load(path, allow_pickle=True)[()]
        meta = dict(artifacts["metadata"])
        if meta.get("dac_version", None) not in SUPPORTED_VERSIONS:
            raise RuntimeError(f"{path} has dac_version {meta.get('dac_version')!r}; this reader knows {SUPPORTED_VERSIONS}")
        return cls(codes=torch.from_numpy(artifacts["codes"].astype(np.int64)), **meta)


def _no_grad_frozen(what: str):
    """torch.no_grad() for a method that has no gradient path, which refuses when set_encode_trainable would have made one expected: the switch
    on, gradients enabled and a parameter of the chosen part requiring one."""
    def deco(fn):
        @functools.wraps(fn)
        def wrapped(self, *args, **kwargs):
            if self._encoder_trains():
                raise NotImplementedError(f"{what} has no parameter gradients (set_encode_trainable({self._encode_trainable!r}) is in effect and a "
                                          "parameter requires grad): call it under torch.no_grad(), or train through encode / forward")
            with torch.no_grad():
                return fn(self, *args, **kwargs)
        return wrapped
    return deco


def _check_device(x: torch.Tensor, what: str):
    if not x.is_cuda:
        raise RuntimeError(f"esc.baselines.DAC runs on the HIP device only: {what} is on {x.device}")


class DAC(nn.Module):
    def __init__(self, encoder_dim: int = 64, encoder_rates: List[int] = [2, 4, 8, 8], latent_dim: int = None, decoder_dim: int = 1536,
                 decoder_rates: List[int] = [8, 8, 4, 2], n_codebooks: int = 9, codebook_size: int = 1024, codebook_dim: Union[int, list] = 8,
                 quantizer_dropout: bool = False, sample_rate: int = 44100):
        super().__init__()
        if not isinstance(codebook_dim, int):
            if len(set(codebook_dim)) != 1:
                raise NotImplementedError("per-codebook codebook_dim lists are not implemented; give one int")
            codebook_dim = int(codebook_dim[0])
        if latent_dim is None:
            latent_dim = encoder_dim * (2 ** len(encoder_rates))
        self.encoder_dim, self.encoder_rates, self.decoder_dim, self.decoder_rates = encoder_dim, list(encoder_rates), decoder_dim, list(decoder_rates)
        self.latent_dim, self.sample_rate = latent_dim, sample_rate
        self.hop_length = int(math.prod(encoder_rates))
        self.n_codebooks, self.codebook_size, self.codebook_dim, self.quantizer_dropout = n_codebooks, codebook_size, codebook_dim, quantizer_dropout
        self.kwargs = dict(encoder_dim=encoder_dim, encoder_rates=list(encoder_rates), latent_dim=latent_dim, decoder_dim=decoder_dim,
                           decoder_rates=list(decoder_rates), n_codebooks=n_codebooks, codebook_size=codebook_size, codebook_dim=codebook_dim,
                           quantizer_dropout=quantizer_dropout, sample_rate=sample_rate)
        for key, shape in _param_specs(encoder_dim, encoder_rates, latent_dim, decoder_dim, decoder_rates, n_codebooks, codebook_size, codebook_dim):
            if key.endswith("alpha"):
                t = torch.ones(shape)
            elif key.endswith("weight_v"):
                t = torch.empty(shape).normal_(0.0, 0.02)            # init_weights: trunc_normal(std 0.02), bias 0 (dac.py:18-21)
            elif key.endswith("weight_g"):
                t = torch.ones(shape)
            elif key.endswith("codebook.weight"):
                t = torch.randn(shape)
            else:
                t = torch.zeros(shape)
            _attach(self, key, t, False)
        with torch.no_grad():                                        # weight_norm's g = ||v|| over every dim but dim 0
            for name, p in self.named_parameters():
                if name.endswith("weight_g"):
                    v = self.get_parameter(name[:-1] + "v")
                    p.copy_(v.flatten(1).norm(dim=1).view(p.shape))
        q = self.quantizer                                           # the reference's `quantizer` holds the parameters and from_codes (quantize.py:200-220)
        q.from_codes, q.n_codebooks, q.codebook_size, q.codebook_dim = self._from_codes, n_codebooks, codebook_size, [codebook_dim] * n_codebooks
        q.forward, q.from_latents = self._quantize, self._from_latents       # quantizer(z, n_quantizers) and from_latents (quantize.py:127-198, 222-255)
        self._handles, self._flat = {}, {}
        self._precision = "fp32"
        self._grad_precision = "fp32"
        self._param_grad_precision = "fp32"
        self._padding = True
        self._trainable = None
        self._encode_trainable = None

    # ---- native handle and flat parameter buffer (same scheme as esc.models.Discriminator) ----------------------------------------------
    def _version(self) -> int:
        return sum(p._version for p in self.parameters())

    def _apply(self, fn, *a, **k):
        self._drop()
        return super()._apply(fn, *a, **k)

    def _drop(self):
        if getattr(self, "_handles", None):
            lib = _native.load()
            for hd in self._handles.values():
                lib.escx_dac_destroy(hd)
        self._handles, self._flat = {}, {}

    def __del__(self):
        try:
            self._drop()
        except Exception:
            pass

    def __getstate__(self):
        st = self.__dict__.copy()
        st["_handles"], st["_flat"] = {}, {}
        return st

    def _handle(self, device):
        lib = _native.load()
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if idx not in self._handles:
            if len(self.encoder_rates) > 8 or len(self.decoder_rates) > 8:
                raise NotImplementedError("more than 8 encoder or decoder rates")
            c = _native.EscxDacConfig()
            c.encoder_dim, c.n_encoder_rates, c.latent_dim = self.encoder_dim, len(self.encoder_rates), self.latent_dim
            c.decoder_dim, c.n_decoder_rates = self.decoder_dim, len(self.decoder_rates)
            for i, s in enumerate(self.encoder_rates):
                c.encoder_rates[i] = s
            for i, s in enumerate(self.decoder_rates):
                c.decoder_rates[i] = s
            c.n_codebooks, c.codebook_size, c.codebook_dim, c.sample_rate = self.n_codebooks, self.codebook_size, self.codebook_dim, self.sample_rate
            hd = ctypes.c_void_p()
            _native.check(lib.escx_dac_create(ctypes.byref(c), idx, ctypes.byref(hd)))
            self._handles[idx] = hd
            if getattr(self, "_snake_maps", None) is not None:
                _native.check(lib.escx_dac_set_snake_maps(hd, self._snake_maps))
            _native.check(lib.escx_dac_set_precision(hd, _native.PRECISIONS[self._precision]))
            _native.check(lib.escx_dac_set_grad_precision(hd, _native.PRECISIONS[self._grad_precision]))
            _native.check(lib.escx_dac_set_param_grad_precision(hd, _native.PRECISIONS[self._param_grad_precision]))
            _native.check(lib.escx_dac_set_padding(hd, int(self._padding)))
        return lib, self._handles[idx]

    def _ensure_flat(self, device, lib, hd):
        """Flat fp32 parameter buffer in the library's order; the nn.Parameters become views of it."""
        idx = device.index if device.index is not None else torch.cuda.current_device()
        st = self._flat.get(idx)
        params = dict(self.named_parameters())
        if st is None:
            n = lib.escx_dac_param_count(hd)
            layout = [(lib.escx_dac_param_key(hd, i).decode(), int(lib.escx_dac_param_offset(hd, i)), int(lib.escx_dac_param_numel(hd, i))) for i in range(n)]
            if [k for k, _, _ in layout] != list(params):
                raise RuntimeError("libescx's DAC parameter order differs from the module's")
            st = {"flat": torch.zeros(int(lib.escx_dac_param_total(hd)), dtype=torch.float32, device=device), "layout": layout}
            self._flat[idx] = st
        flat, base = st["flat"], st["flat"].data_ptr()
        with torch.no_grad():
            for key, off, n in st["layout"]:
                p = params[key]
                if p.data_ptr() != base + 4 * off:
                    flat[off:off + n].copy_(p.detach().reshape(-1).to(device=device, dtype=torch.float32))
                    p.data = flat[off:off + n].view(p.shape)
        return flat

    def _ctx(self, x: torch.Tensor, what: str):
        if self.training:
            raise NotImplementedError("esc.baselines.DAC is inference only: call .eval() (DAC training is not implemented)")
        _check_device(x, what)
        dev = x.device
        lib, hd = self._handle(dev)
        flat = self._ensure_flat(dev, lib, hd)
        return lib, hd, flat, dev, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def set_snake_maps(self, mask: int):
        """Where Snake is evaluated per layer class (include/escx.h escx_dac_set_snake_maps; bitwise the same results either way).  A/B aid."""
        self._snake_maps = int(mask)
        for hd in self._handles.values():
            _native.check(_native.load().escx_dac_set_snake_maps(hd, self._snake_maps))
        return self

    # ---- arithmetic of the convolutions (include/escx.h escx_dac_set_precision) --------------------------------------------------------------
    def set_precision(self, mode: str) -> "DAC":
        """Operand form of the convolutions of encode / decode / eval forward, with ESC.set_precision's names: "fp32" (fp32 MFMA, the default, the
        reference's operand precision) or "bf16x3" (every fp32 operand split exactly into three bf16 terms, six cross products accumulated in
        fp32: fp32-grade results up to summation order, on the 16-bit matrix cores).  "f16x2" is refused: two fp16 terms need a bound on every
        operand and Snake outputs have none.  The quantiser is fp32 in both modes.  Not part of the reference's surface."""
        if mode not in _native.PRECISIONS:
            raise ValueError(f"precision {mode!r}: expected one of {sorted(_native.PRECISIONS)}")
        if mode == "f16x2":
            raise NotImplementedError("DAC has no f16x2 mode: two fp16 terms need an a-priori bound on every operand (csrc/split_terms.h) and Snake "
                                      "outputs have none; use bf16x3, which keeps fp32's exponent range and needs no bound")
        self._precision = mode
        for hd in self._handles.values():
            _native.check(_native.load().escx_dac_set_precision(hd, _native.PRECISIONS[mode]))
        return self

    @property
    def precision(self) -> str:
        """The mode in effect: what set_precision chose ("fp32" until then); every live handle is in it."""
        return self._precision

    # ---- arithmetic of the backward (include/escx.h escx_dac_set_grad_precision) ---------------------------------------------------------------
    def set_grad_precision(self, mode: str) -> "DAC":
        """Operand form of the backward of decode / encode / forward, with set_precision's names and independent of it: "fp32" (fp32 MFMA, the
        default, today's bits) or "bf16x3" (the input gradient of every convolution of the decoder and the encoder on the 16-bit matrix cores:
        output gradient and transposed weights split exactly into three bf16 terms, six cross products accumulated in fp32 in two levels).  The
        decoder's weight-gradient contractions (set_param_grad_precision's) and the quantiser's backward (fp32) do not follow this switch.  "f16x2" is refused: two fp16 terms need a
        bound on every operand, and neither output gradients nor Snake outputs have one.  The mode is read when backward runs, not when the
        graph was made; forward values never depend on it.  Not part of the reference's surface."""
        if not isinstance(mode, str) or mode not in _native.PRECISIONS:
            raise ValueError(f"grad precision {mode!r}: expected one of {sorted(_native.PRECISIONS)}")
        if mode == "f16x2":
            raise NotImplementedError("DAC has no f16x2 backward: two fp16 terms need an a-priori bound on every operand (csrc/split_terms.h) and "
                                      "neither output gradients nor Snake outputs have one; use bf16x3, which keeps fp32's exponent range")
        self._grad_precision = mode
        for hd in self._handles.values():
            _native.check(_native.load().escx_dac_set_grad_precision(hd, _native.PRECISIONS[mode]))
        return self

    @property
    def grad_precision(self) -> str:
        """The backward's mode in effect: what set_grad_precision chose ("fp32" until then); every live handle is in it."""
        return self._grad_precision

    # ---- arithmetic of the weight gradients (include/escx.h escx_dac_set_param_grad_precision) ------------------------------------------------
    def set_param_grad_precision(self, mode: str) -> "DAC":
        """Operand form of the decoder's weight-gradient contractions after set_trainable("decoder"), with set_precision's names and independent
        of set_precision and set_grad_precision: "fp32" (fp32 MFMA, the default, today's bits) or "bf16x3" (the dW contraction of every decoder
        convolution with more than one input and more than one output channel on the 16-bit matrix cores: output-gradient rows and Snaked input
        rows split exactly into three bf16 terms, six cross products accumulated in fp32, the row slices added in increasing order; 128 x 128
        tiles of dW, 64 or 32 x 128 for layers of at most 64 channels).  The
        one-channel last convolution, the bias / alpha column sums and the weight norm's backward are the same in both modes, and so are the
        audio and d_z.  "f16x2" is refused: two fp16 terms need a bound on every operand, and neither output gradients nor Snake outputs have
        one.  The mode is read when backward runs, not when the graph was made.  Not part of the reference's surface."""
        if not isinstance(mode, str) or mode not in _native.PRECISIONS:
            raise ValueError(f"param grad precision {mode!r}: expected one of {sorted(_native.PRECISIONS)}")
        if mode == "f16x2":
            raise NotImplementedError("DAC has no f16x2 weight gradient: two fp16 terms need an a-priori bound on every operand (csrc/split_terms.h) "
                                      "and neither output gradients nor Snake outputs have one; use bf16x3, which keeps fp32's exponent range")
        self._param_grad_precision = mode
        for hd in self._handles.values():
            _native.check(_native.load().escx_dac_set_param_grad_precision(hd, _native.PRECISIONS[mode]))
        return self

    @property
    def param_grad_precision(self) -> str:
        """The weight gradients' mode in effect: what set_param_grad_precision chose ("fp32" until then); every live handle is in it."""
        return self._param_grad_precision

    # ---- fine-tuning the decoder (include/escx.h escx_dac_decode_backward_params) ----------------------------------------------------------------
    def set_trainable(self, part: Optional[str]) -> "DAC":
        """Which part of the model `decode` differentiates with respect to its parameters.  None (the default): none, today's behaviour bit for
        bit.  "decoder": in eval mode, with padding on and gradients enabled, decode(z) delivers through autograd the gradient of every decoder
        parameter that requires one (and of z if it requires one); the audio is bitwise the plain decode's.  The decoder has no train / eval
        difference, so the model stays in eval mode; `.train()` still refuses.  This is `decode`'s switch: the encoder's and the quantiser's
        parameters are `encode`'s and have their own, set_encode_trainable, so "encoder", "quantizer" and "all" raise NotImplementedError here."""
        if part in ("encoder", "quantizer", "all"):
            raise NotImplementedError(f"set_trainable({part!r}): this is decode's switch and takes None or 'decoder'; the encoder's and the quantiser's "
                                      "parameter gradients are encode's: set_encode_trainable('encoder' | 'quantizer' | 'both'), next to "
                                      "set_trainable('decoder') for the whole model (quantiser dropout and training mode are not built)")
        if part not in (None, "decoder"):
            raise ValueError(f"set_trainable({part!r}): expected None or 'decoder'")
        self._trainable = part
        return self

    @property
    def trainable(self) -> Optional[str]:
        """What set_trainable chose: None or "decoder"."""
        return self._trainable

    def decoder_parameters(self):
        """The `decoder.*` parameters in state_dict order: what an optimiser fine-tunes after set_trainable("decoder")."""
        for key, p in self.named_parameters():
            if key.startswith("decoder."):
                yield p

    # ---- fine-tuning the encoder and the quantiser (include/escx.h escx_dac_encode_backward_params) ----------------------------------------------
    def set_encode_trainable(self, part: Optional[str]) -> "DAC":
        """Which part of the model `encode` differentiates with respect to its parameters, independent of set_trainable.  None (the default):
        none, today's behaviour bit for bit.  "encoder", "quantizer" or "both": in eval mode, with padding on and gradients enabled,
        encode(x, n_quantizers) delivers through autograd the gradient of every parameter of the chosen part that requires one (and of x if it
        requires one, bitwise the frozen path's); the forward values are bitwise the plain encode's.  With the quantiser chosen the codebook loss
        is differentiable with respect to the codebooks.  A quantiser stage that no clip of the call runs gets no gradient (None), as under
        torch autograd of the reference.  With set_trainable("decoder") next to "both", forward(x) delivers the gradient of every parameter of
        the model.  The model stays in eval mode; `.train()` still refuses, and quantiser dropout is per-clip n_quantizers sampled by the caller.
        Anything else raises ValueError and leaves the switch as it was.  Never touches a device."""
        if not (part is None or (isinstance(part, str) and part in _ENCODE_PARTS)):
            raise ValueError(f"set_encode_trainable({part!r}): expected None, 'encoder', 'quantizer' or 'both'")
        self._encode_trainable = part
        return self

    @property
    def encode_trainable(self) -> Optional[str]:
        """What set_encode_trainable chose: None, "encoder", "quantizer" or "both"."""
        return self._encode_trainable

    def encoder_parameters(self):
        """The `encoder.*` parameters in state_dict order."""
        for key, p in self.named_parameters():
            if key.startswith("encoder."):
                yield p

    def quantizer_parameters(self):
        """The `quantizer.*` parameters in state_dict order (per stage: in_proj, out_proj, codebook)."""
        for key, p in self.named_parameters():
            if key.startswith("quantizer."):
                yield p

    def _encode_named(self):
        """[(key, parameter)] of the part set_encode_trainable chose, in state_dict order."""
        prefixes = {"encoder": ("encoder.",), "quantizer": ("quantizer.",), "both": ("encoder.", "quantizer.")}[self._encode_trainable]
        return [(k, p) for k, p in self.named_parameters() if k.startswith(prefixes)]

    def _encoder_trains(self) -> bool:
        return self._encode_trainable is not None and torch.is_grad_enabled() and any(p.requires_grad for _, p in self._encode_named())

    # ---- CodecMixin's padding switch and geometry (base.py:58-123) ----------------------------------------------------------------------
    @property
    def padding(self) -> bool:
        """True (the default): every convolution pads as constructed.  False: every Conv1d / ConvTranspose1d runs with padding 0 and a
        ResidualUnit adds its input cropped by 3 * dilation on each side, as the reference's layers do after `model.padding = False`
        (include/escx.h escx_dac_set_padding).  encode / decode / num_frames / output_samples follow the mode."""
        return self._padding

    @padding.setter
    def padding(self, value):
        assert isinstance(value, bool)
        self._padding = value
        for hd in self._handles.values():
            _native.check(_native.load().escx_dac_set_padding(hd, int(value)))

    @property
    def device(self):
        return next(self.parameters()).device

    def _conv_layers(self):
        """(transposed, kernel, stride, dilation) of every convolution of encoder and decoder in module order.  The quantiser's 1x1 projections
        lie between them and change no length."""
        out = [(False, 7, 1, 1)]
        for s in self.encoder_rates:
            for d in (1, 3, 9):
                out += [(False, 7, 1, d), (False, 1, 1, 1)]
            out.append((False, 2 * s, s, 1))
        out += [(False, 3, 1, 1), (False, 7, 1, 1)]
        for s in self.decoder_rates:
            out.append((True, 2 * s, s, 1))
            for d in (1, 3, 9):
                out += [(False, 7, 1, d), (False, 1, 1, 1)]
        out.append((False, 7, 1, 1))
        return out

    def get_output_length(self, input_length: int) -> int:
        """base.py:108-123: samples out of encoder + decoder for input_length in with every convolution unpadded, floored at each layer (the
        reference evaluates it at 0, where it is negative).  It is the hop between chunks of `compress`."""
        L = int(input_length)
        for tr, k, s, d in self._conv_layers():
            reach = d * (k - 1) + 1
            L = (L - 1) * s + reach if tr else (L - reach) // s + 1
        return L

    def get_delay(self) -> int:
        """base.py:82-106: half of what the unpadded model's receptive field takes off a signal; `compress` zero-pads by it on both sides."""
        l_out = self.get_output_length(0)
        L = l_out
        for tr, k, s, d in reversed(self._conv_layers()):
            reach = d * (k - 1) + 1
            L = -((reach - L) // s) + 1 if tr else (L - 1) * s + reach
        return (L - l_out) // 2

    @property
    def delay(self) -> int:
        return self.get_delay()

    def _walk(self, t: int, layers) -> int:
        """Length after `layers` without padding; 0 as soon as one of them would give no row."""
        for tr, k, s, d in layers:
            reach = d * (k - 1) + 1
            t = (t - 1) * s + reach if tr else ((t - reach) // s + 1 if t >= reach else 0)
            if t < 1:
                return 0
        return t

    # ---- length arithmetic ---------------------------------------------------------------------------------------------------------------
    def num_frames(self, n_samples: int) -> int:
        """Latent frames of an n_samples clip (torch's Conv1d length formula through the encoder); 0 when the clip is shorter than one hop
        (with `padding` off: shorter than the encoder's receptive field)."""
        t = int(n_samples)
        if not self._padding:
            return self._walk(t, self._conv_layers()[:2 + 7 * len(self.encoder_rates)]) if t >= 1 else 0
        for s in self.encoder_rates:
            t = (t + 2 * math.ceil(s / 2) - 2 * s) // s + 1
            if t < 1:
                return 0
        return t

    def output_samples(self, n_frames: int) -> int:
        """Samples decoded from n_frames latent frames: 320 T - 8 for rates [8, 5, 4, 2]; with `padding` off the unpadded decoder's (0: none)."""
        t = int(n_frames)
        if not self._padding:
            return self._walk(t, self._conv_layers()[2 + 7 * len(self.encoder_rates):]) if t >= 1 else 0
        for s in self.decoder_rates:
            t = (t - 1) * s - 2 * math.ceil(s / 2) + 2 * s
        return t

    # ---- the reference's interface -------------------------------------------------------------------------------------------------------
    def preprocess(self, audio_data, sample_rate):
        if sample_rate is None:
            sample_rate = self.sample_rate
        if sample_rate != self.sample_rate:
            raise AssertionError(f"sample_rate {sample_rate} != the model's {self.sample_rate}")
        length = audio_data.shape[-1]
        right_pad = math.ceil(length / self.hop_length) * self.hop_length - length
        return nn.functional.pad(audio_data, (0, right_pad))

    def sample_n_quantizers(self, batch: int, generator: Optional[torch.Generator] = None) -> List[int]:
        """The reference's training-mode quantiser dropout (nn/quantize.py:166-171) as per-clip counts for encode / forward: the first
        int(batch * quantizer_dropout) clips get randint(1, n_codebooks + 1), the rest all n_codebooks.  One draw per clip of the batch, as the
        reference makes them (on the CPU; `generator` seeds it)."""
        batch = int(batch)
        if batch < 1:
            raise ValueError(f"batch must be at least 1, got {batch}")
        dropout = torch.randint(1, self.n_codebooks + 1, (batch,), generator=generator)
        n_dropout = int(batch * self.quantizer_dropout)
        return [int(v) for v in dropout[:n_dropout].tolist()] + [self.n_codebooks] * (batch - n_dropout)

    def _n_quantizers(self, n_quantizers):
        if n_quantizers is None:
            return self.n_codebooks
        n = int(n_quantizers)
        if n < 1:
            raise ValueError(f"n_quantizers must be at least 1, got {n_quantizers}")
        return min(n, self.n_codebooks)                 # the reference's loop stops at the last codebook

    @staticmethod
    def _int_entries(n_quantizers, what: str) -> List[int]:
        """The entries of a sequence or 1-D integer tensor of codebook counts as Python ints; anything else raises ValueError."""
        if isinstance(n_quantizers, torch.Tensor):
            if n_quantizers.dim() != 1 or n_quantizers.is_floating_point() or n_quantizers.is_complex() or n_quantizers.dtype == torch.bool:
                raise ValueError(f"{what} must be a 1-D integer tensor, got {n_quantizers.dtype} of shape {tuple(n_quantizers.shape)}")
            return [int(v) for v in n_quantizers.tolist()]
        vals = list(n_quantizers)
        for v in vals:
            if isinstance(v, torch.Tensor) and v.dim() == 0 and not (v.is_floating_point() or v.is_complex() or v.dtype == torch.bool):
                continue
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"{what} must hold integers, got {v!r}")
        return [int(v) for v in vals]

    @staticmethod
    def _is_per_clip(n_quantizers) -> bool:
        return isinstance(n_quantizers, (list, tuple, np.ndarray)) or (isinstance(n_quantizers, torch.Tensor) and n_quantizers.dim() >= 1)

    def _clip_counts(self, n_quantizers, batch: int) -> List[int]:
        """Per-clip codebook counts (the per-item mask of quantize.py:181-190): `batch` integers, each at least 1, clamped to n_codebooks."""
        vals = self._int_entries(n_quantizers, "per-clip n_quantizers")
        if len(vals) != batch:
            raise ValueError(f"per-clip n_quantizers has {len(vals)} entries for a batch of {batch}")
        for v in vals:
            if v < 1:
                raise ValueError(f"n_quantizers must be at least 1 for every clip, got {v}")
        return [min(v, self.n_codebooks) for v in vals]

    def _sweep_counts(self, n_quantizers) -> List[int]:
        """encode_sweep's stage counts: strictly increasing integers from 1 up, each clamped to n_codebooks; duplicates after the clamp raise."""
        if not self._is_per_clip(n_quantizers):
            raise ValueError("encode_sweep takes a sequence of codebook counts")
        vals = self._int_entries(n_quantizers, "encode_sweep's n_quantizers")
        if not vals:
            raise ValueError("encode_sweep needs at least one codebook count")
        if vals[0] < 1:
            raise ValueError(f"n_quantizers must be at least 1, got {vals[0]}")
        if any(b <= a for a, b in zip(vals, vals[1:])):
            raise ValueError(f"encode_sweep's n_quantizers must be strictly increasing, got {vals}")
        out = [min(v, self.n_codebooks) for v in vals]
        if len(set(out)) != len(out):
            raise ValueError(f"encode_sweep's n_quantizers {vals} repeat a count once clamped to the {self.n_codebooks} codebooks")
        return out

    # ---- mixed-length batches: one length per clip (include/escx.h escx_dac_encode_lengths and its two neighbours) --------------------------
    def _clip_lengths(self, lengths, batch: int, hi: int, what: str) -> List[int]:
        """Per-clip lengths: `batch` integers in [1, hi], read with the helper (and the messages) of the per-clip codebook counts."""
        vals = self._int_entries(lengths, what)
        if len(vals) != batch:
            raise ValueError(f"{what} has {len(vals)} entries for a batch of {batch}")
        for b, v in enumerate(vals):
            if v < 1 or v > hi:
                raise ValueError(f"{what}[{b}] = {v} outside [1, {hi}]")
        return vals

    def _refuse_lengths(self, what: str, grad: bool):
        """The calls per-clip lengths do not cover, refused before anything is launched."""
        if not self._padding:
            raise NotImplementedError(f"{what} needs padding = True: with the padding off every clip loses the receptive field at both ends and "
                                      "the chunked path batches equal windows already")
        if grad:
            raise NotImplementedError(f"{what} is not implemented on the gradient paths (an input that requires grad, or set_trainable('decoder') / "
                                      "set_encode_trainable with a parameter that requires grad): call it under torch.no_grad() or differentiate clip by clip")

    def _decoder_trains(self) -> bool:
        return self._trainable == "decoder" and torch.is_grad_enabled() and any(p.requires_grad for p in self.decoder_parameters())

    def frame_lengths(self, lengths) -> torch.Tensor:
        """num_frames of every entry of `lengths` (a sequence or 1-D integer tensor of sample counts): a 1-D int64 CPU tensor."""
        return torch.tensor([self.num_frames(v) for v in self._int_entries(lengths, "lengths")], dtype=torch.int64)

    def output_lengths(self, frame_lengths) -> torch.Tensor:
        """output_samples of every entry of `frame_lengths`: a 1-D int64 CPU tensor."""
        return torch.tensor([self.output_samples(v) for v in self._int_entries(frame_lengths, "frame_lengths")], dtype=torch.int64)

    def _check_encode_lengths(self, audio_data, lengths, pad_multiple: int):
        """(lengths, frames per clip) of an encode with per-clip lengths; every clip must give a frame once padded to a multiple of pad_multiple."""
        if not isinstance(audio_data, torch.Tensor) or audio_data.dim() != 3 or audio_data.shape[1] != 1:
            raise ValueError(f"audio_data must be (B, 1, L), got {tuple(getattr(audio_data, 'shape', ()))}")
        B, _, L = audio_data.shape
        lens = self._clip_lengths(lengths, B, L, "lengths")
        frames = [self.num_frames(-(-v // pad_multiple) * pad_multiple) for v in lens]
        for b, (v, t) in enumerate(zip(lens, frames)):
            if t < 1:
                raise ValueError(f"lengths[{b}] = {v} samples are shorter than one hop ({self.hop_length}): the encoder gives no frame for clip {b}")
        return lens, frames

    @torch.no_grad()
    def _encode_lengths(self, audio_data: torch.Tensor, lens: List[int], frames: List[int], n_quantizers, pad_multiple: int):
        """encode of clips of their own lengths (include/escx.h escx_dac_encode_lengths), each right-padded with staged zeros to a multiple of
        pad_multiple."""
        counts = self._clip_counts(n_quantizers, audio_data.shape[0]) if self._is_per_clip(n_quantizers) else None
        n = self._n_quantizers(n_quantizers) if counts is None else max(counts)
        lib, hd, flat, dev, stream = self._ctx(audio_data, "audio_data")
        B, _, L = audio_data.shape
        T = max(frames)
        x = audio_data.to(torch.float32).contiguous()
        z = torch.empty(B, self.latent_dim, T, device=dev)
        codes = torch.empty(B, n, T, dtype=torch.int64, device=dev)
        latents = torch.empty(B, n * self.codebook_dim, T, device=dev)
        losses = torch.empty(2, device=dev)
        cn = (ctypes.c_int32 * B)(*counts) if counts is not None else None
        with torch.cuda.device(dev):
            _native.check(lib.escx_dac_encode_lengths(hd, ctypes.c_void_p(flat.data_ptr()), self._version(), ctypes.c_void_p(x.data_ptr()), B, L,
                                                      (ctypes.c_int32 * B)(*lens), pad_multiple, n, cn, ctypes.c_void_p(z.data_ptr()),
                                                      ctypes.c_void_p(codes.data_ptr()), ctypes.c_void_p(latents.data_ptr()),
                                                      ctypes.c_void_p(losses.data_ptr()), stream))
        return z, codes, latents, losses[0], losses[1]

    def _check_frame_lengths(self, t: torch.Tensor, frame_lengths, what: str) -> List[int]:
        if not isinstance(t, torch.Tensor) or t.dim() != 3:
            raise ValueError(f"{what} must be 3-D, got {tuple(getattr(t, 'shape', ()))}")
        fl = self._clip_lengths(frame_lengths, t.shape[0], t.shape[-1], "frame_lengths")
        for b, v in enumerate(fl):
            if self.output_samples(v) < 1:
                raise ValueError(f"frame_lengths[{b}] = {v} latent frames decode to no sample for clip {b}")
        return fl

    @torch.no_grad()
    def _decode_lengths(self, z: torch.Tensor, fl: List[int], caps: Optional[List[int]] = None):
        """decode of clips of their own frame counts (include/escx.h escx_dac_decode_lengths); caps: cut clip b's audio at caps[b] samples."""
        lib, hd, flat, dev, stream, B, T, n_out = self._decode_args(z)
        zc = z.to(torch.float32).contiguous()
        out = torch.empty(B, 1, n_out, device=dev)
        with torch.cuda.device(dev):
            _native.check(lib.escx_dac_decode_lengths(hd, ctypes.c_void_p(flat.data_ptr()), self._version(), ctypes.c_void_p(zc.data_ptr()), B, T,
                                                      (ctypes.c_int32 * B)(*fl), None if caps is None else (ctypes.c_int32 * B)(*caps),
                                                      ctypes.c_void_p(out.data_ptr()), stream))
        return out

    def _audio_shape(self, audio_data):
        if audio_data.dim() != 3 or audio_data.shape[1] != 1:
            raise ValueError(f"audio_data must be (B, 1, L), got {tuple(audio_data.shape)}")
        B, _, L = audio_data.shape
        T = self.num_frames(L)
        if T < 1:
            raise ValueError(f"{L} samples are shorter than one hop ({self.hop_length}): the encoder gives no frame")
        return B, L, T

    @torch.no_grad()
    def _encode_counts(self, audio_data: torch.Tensor, counts: List[int]):
        """encode with one codebook count per clip (include/escx.h escx_dac_encode_ex, clip_n)."""
        lib, hd, flat, dev, stream = self._ctx(audio_data, "audio_data")
        B, L, T = self._audio_shape(audio_data)
        n = max(counts)
        x = audio_data.to(torch.float32).contiguous()
        z = torch.empty(B, self.latent_dim, T, device=dev)
        codes = torch.empty(B, n, T, dtype=torch.int64, device=dev)
        latents = torch.empty(B, n * self.codebook_dim, T, device=dev)
        losses = torch.empty(2, device=dev)
        cn = (ctypes.c_int32 * B)(*counts)
        with torch.cuda.device(dev):
            _native.check(lib.escx_dac_encode_ex(hd, ctypes.c_void_p(flat.data_ptr()), self._version(), ctypes.c_void_p(x.data_ptr()), B, L, n, cn, None, 0,
                                                 ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(codes.data_ptr()), ctypes.c_void_p(latents.data_ptr()),
                                                 ctypes.c_void_p(losses.data_ptr()), None, stream))
        return z, codes, latents, losses[0], losses[1]

    @_no_grad_frozen("encode_sweep")
    def encode_sweep(self, audio_data: torch.Tensor, n_quantizers: Sequence[int], lengths=None):
        """One encode for a whole bitrate sweep: (zs (R, B, D, T), codes (B, n_max, T), latents (B, n_max d, T)) with zs[r] bitwise the z of
        encode(audio_data, n_quantizers[r]) and codes / latents those of the largest count (the codes are prefix codes; the quantiser stores its
        running sum, quantize.py:185, after each requested stage: include/escx.h escx_dac_encode_ex, snap_n).  Not part of the reference's surface."""
        if self.training:
            raise NotImplementedError("esc.baselines.DAC is inference only: call .eval() (DAC training is not implemented)")
        if lengths is not None:
            raise NotImplementedError("encode_sweep takes no per-clip lengths: the snapshots are built for uniform batches (use encode with lengths, "
                                      "one call per bitrate)")
        ns = self._sweep_counts(n_quantizers)
        lib, hd, flat, dev, stream = self._ctx(audio_data, "audio_data")
        B, L, T = self._audio_shape(audio_data)
        n, R = ns[-1], len(ns)
        x = audio_data.to(torch.float32).contiguous()
        z = torch.empty(B, self.latent_dim, T, device=dev)
        zs = torch.empty(R, B, self.latent_dim, T, device=dev)
        codes = torch.empty(B, n, T, dtype=torch.int64, device=dev)
        latents = torch.empty(B, n * self.codebook_dim, T, device=dev)
        losses = torch.empty(2, device=dev)
        sn = (ctypes.c_int32 * R)(*ns)
        with torch.cuda.device(dev):
            _native.check(lib.escx_dac_encode_ex(hd, ctypes.c_void_p(flat.data_ptr()), self._version(), ctypes.c_void_p(x.data_ptr()), B, L, n, None, sn, R,
                                                 ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(codes.data_ptr()), ctypes.c_void_p(latents.data_ptr()),
                                                 ctypes.c_void_p(losses.data_ptr()), ctypes.c_void_p(zs.data_ptr()), stream))
        return zs, codes, latents

    def encode(self, audio_data: torch.Tensor, n_quantizers: Union[int, Sequence[int], torch.Tensor] = None, lengths=None):
        """dac.py:209-247: (z (B, D, T), codes (B, n, T) int64, latents (B, n d, T), commitment_loss, codebook_loss).  n_quantizers may also be
        one count per clip (a sequence or 1-D integer tensor of B entries, the per-item mask of quantize.py:181-190): n = max(counts), codes hold
        -1 and latents 0 past a clip's count, the losses are the reference's masked means.  When gradients are enabled and audio_data requires
        one, z, latents and commitment_loss carry the audio gradient of the reference's eval-mode autograd (straight-through quantiser,
        quantize.py:58-70; eval mode, padding on; `_EncodeGrad` below): the same bits, computed by escx_dac_encode_tape, which keeps the
        encoder's maps in a tape on the graph.  The module's parameters get no gradient whatever their requires_grad, unless
        set_encode_trainable is in effect: then every parameter of the chosen part that requires a gradient gets one, x may or may not
        require one, and with the quantiser chosen codebook_loss is differentiable in the codebooks (`_EncodeParamGrad`).

        lengths (a sequence or 1-D integer tensor, one sample count in [1, L] per clip; not part of the reference's surface) makes the batch a
        mixed-length one: clip b's results are bitwise those of encode(audio_data[b:b+1, :, :lengths[b]]) alone, nothing at or past a clip's
        length is read, and the tuple comes at Tmax = num_frames(max(lengths)) with z and latents 0 and codes -1 at frames >=
        num_frames(lengths[b]).  The losses are the means over the clips of the single-clip calls' losses.  Combines with per-clip
        n_quantizers; padding on, no gradients."""
        if self.training:
            raise NotImplementedError("esc.baselines.DAC is inference only: call .eval() (DAC training is not implemented)")
        if lengths is not None:
            self._refuse_lengths("encode with lengths",
                                 (torch.is_grad_enabled() and isinstance(audio_data, torch.Tensor) and audio_data.requires_grad) or self._encoder_trains())
            lens, frames = self._check_encode_lengths(audio_data, lengths, 1)
            if self._is_per_clip(n_quantizers):
                self._clip_counts(n_quantizers, audio_data.shape[0])
            return self._encode_lengths(audio_data, lens, frames, n_quantizers, 1)
        if isinstance(audio_data, torch.Tensor) and self._encoder_trains():
            counts = self._clip_counts(n_quantizers, audio_data.shape[0]) if self._is_per_clip(n_quantizers) else None
            named = self._encode_named()
            return _EncodeParamGrad.apply(audio_data, self, self._n_quantizers(n_quantizers) if counts is None else max(counts), counts,
                                          tuple(k for k, _ in named), *[p for _, p in named])
        if torch.is_grad_enabled() and isinstance(audio_data, torch.Tensor) and audio_data.requires_grad:
            counts = self._clip_counts(n_quantizers, audio_data.shape[0]) if self._is_per_clip(n_quantizers) else None
            return _EncodeGrad.apply(audio_data, self, self._n_quantizers(n_quantizers) if counts is None else max(counts), counts)
        with torch.no_grad():
            return self._encode(audio_data, n_quantizers)

    def _encode(self, audio_data: torch.Tensor, n_quantizers):
        if self._is_per_clip(n_quantizers):
            return self._encode_counts(audio_data, self._clip_counts(n_quantizers, audio_data.shape[0]))
        lib, hd, flat, dev, stream = self._ctx(audio_data, "audio_data")
        n = self._n_quantizers(n_quantizers)
        if audio_data.dim() != 3 or audio_data.shape[1] != 1:
            raise ValueError(f"audio_data must be (B, 1, L), got {tuple(audio_data.shape)}")
        B, _, L = audio_data.shape
        T = self.num_frames(L)
        if T < 1:
            raise ValueError(f"{L} samples are shorter than one hop ({self.hop_length}): the encoder gives no frame")
        if not self._padding and lib.escx_dac_num_frames(hd, L) != T:
            raise RuntimeError(f"libescx encodes {L} unpadded samples to {lib.escx_dac_num_frames(hd, L)} frames, the host to {T}")
        x = audio_data.to(torch.float32).contiguous()
        z = torch.empty(B, self.latent_dim, T, device=dev)
        codes = torch.empty(B, n, T, dtype=torch.int64, device=dev)
        latents = torch.empty(B, n * self.codebook_dim, T, device=dev)
        losses = torch.empty(2, device=dev)
        with torch.cuda.device(dev):
            _native.check(lib.escx_dac_encode(hd, ctypes.c_void_p(flat.data_ptr()), self._version(), ctypes.c_void_p(x.data_ptr()), B, L, n,
                                              ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(codes.data_ptr()), ctypes.c_void_p(latents.data_ptr()),
                                              ctypes.c_void_p(losses.data_ptr()), stream))
        return z, codes, latents, losses[0], losses[1]

    def decode(self, z: torch.Tensor, frame_lengths=None):
        """dac.py:249-266: z (B, D, T) -> audio (B, 1, output_samples(T)).  When gradients are enabled and z requires one, the result carries
        the latent gradient d audio / d z (eval mode, padding on; `_DecodeGrad` below): the same audio bits, computed by escx_dac_decode_tape,
        which keeps the decoder's maps in a tape on the graph.  The module's parameters get no gradient whatever their requires_grad, unless
        set_trainable("decoder") is in effect: then every decoder parameter that requires a gradient gets one (`_DecodeParamGrad`).

        frame_lengths (one frame count in [1, T] per clip; not part of the reference's surface): clip b of the (B, 1, output_samples(T)) result is
        bitwise decode(z[b:b+1, :, :frame_lengths[b]]) and 0 from sample output_samples(frame_lengths[b]) on; the frames at or past a clip's
        count are not read.  Padding on, no gradients."""
        if self.training:
            raise NotImplementedError("esc.baselines.DAC is inference only: call .eval() (DAC training is not implemented)")
        if frame_lengths is not None:
            self._refuse_lengths("decode with frame_lengths",
                                 (torch.is_grad_enabled() and isinstance(z, torch.Tensor) and z.requires_grad) or self._decoder_trains())
            fl = self._check_frame_lengths(z, frame_lengths, "z")
            return self._decode_lengths(z, fl)
        if self._trainable == "decoder" and torch.is_grad_enabled() and isinstance(z, torch.Tensor):
            params = list(self.decoder_parameters())
            if any(p.requires_grad for p in params):
                return _DecodeParamGrad.apply(z, self, *params)
        if torch.is_grad_enabled() and isinstance(z, torch.Tensor) and z.requires_grad:
            return _DecodeGrad.apply(z, self)
        with torch.no_grad():
            return self._decode(z)

    def _decode_args(self, z: torch.Tensor):
        """decode's checks: (lib, hd, flat, dev, stream, B, T, n_out)."""
        lib, hd, flat, dev, stream = self._ctx(z, "z")
        if z.dim() != 3 or z.shape[1] != self.latent_dim:
            raise ValueError(f"z must be (B, {self.latent_dim}, T), got {tuple(z.shape)}")
        B, _, T = z.shape
        n_out = self.output_samples(T)
        if n_out < 1:
            raise ValueError(f"{T} latent frames decode to no sample with padding off")
        if not self._padding and lib.escx_dac_output_samples(hd, T) != n_out:
            raise RuntimeError(f"libescx decodes {T} unpadded frames to {lib.escx_dac_output_samples(hd, T)} samples, the host to {n_out}")
        return lib, hd, flat, dev, stream, B, T, n_out

    def _decode(self, z: torch.Tensor):
        lib, hd, flat, dev, stream, B, T, n_out = self._decode_args(z)
        zc = z.to(torch.float32).contiguous()
        out = torch.empty(B, 1, n_out, device=dev)
        with torch.cuda.device(dev):
            _native.check(lib.escx_dac_decode(hd, ctypes.c_void_p(flat.data_ptr()), self._version(), ctypes.c_void_p(zc.data_ptr()), B, T,
                                              ctypes.c_void_p(out.data_ptr()), stream))
        return out

    @torch.no_grad()
    def _from_codes(self, codes: torch.Tensor, n_quantizers: Union[Sequence[int], torch.Tensor] = None, frame_lengths=None):
        """ResidualVectorQuantize.from_codes: (z_q (B, D, T), z_p (B, n d, T), codes); `model.quantizer.from_codes` is this method.  With
        n_quantizers (one count per clip, as encode takes them) clip b sums its first n_b codebooks and the slots past its count are ignored,
        whatever they hold (encode's per-clip form writes -1 there); z_p is 0 in them.  With frame_lengths (one frame count per clip, as decode
        takes them) the slots at frames >= frame_lengths[b] are neither read nor range-checked (encode with lengths writes -1 there) and z_q and
        z_p are 0 there."""
        fl = None
        if frame_lengths is not None:
            if self.training:
                raise NotImplementedError("esc.baselines.DAC is inference only: call .eval() (DAC training is not implemented)")
            self._refuse_lengths("from_codes with frame_lengths", False)
            if not isinstance(codes, torch.Tensor) or codes.dim() != 3:
                raise ValueError(f"codes must be (B, n <= {self.n_codebooks}, T), got {tuple(getattr(codes, 'shape', ()))}")
            fl = self._clip_lengths(frame_lengths, codes.shape[0], codes.shape[-1], "frame_lengths")
        counts = None
        if n_quantizers is not None:
            if self.training:
                raise NotImplementedError("esc.baselines.DAC is inference only: call .eval() (DAC training is not implemented)")
            counts = self._clip_counts(n_quantizers if self._is_per_clip(n_quantizers) else [n_quantizers] * codes.shape[0], codes.shape[0])
        lib, hd, flat, dev, stream = self._ctx(codes, "codes")
        if codes.dim() != 3 or not 1 <= codes.shape[1] <= self.n_codebooks:
            raise ValueError(f"codes must be (B, n <= {self.n_codebooks}, T), got {tuple(codes.shape)}")
        B, n, T = codes.shape
        c = codes.to(torch.int64).contiguous()
        if counts is not None and max(counts) > n:
            raise ValueError(f"per-clip n_quantizers up to {max(counts)} for codes of {n} codebooks")
        used = c
        if counts is not None or fl is not None:                 # the range check covers the slots that are read
            live = torch.ones(1, 1, 1, dtype=torch.bool, device=dev)
            if counts is not None:
                live = live & (torch.arange(n, device=dev)[None, :, None] < torch.tensor(counts, device=dev)[:, None, None])
            if fl is not None:
                live = live & (torch.arange(T, device=dev)[None, None, :] < torch.tensor(fl, device=dev)[:, None, None])
            used = c[live.expand_as(c)]
        if used.numel() and (int(used.min()) < 0 or int(used.max()) >= self.codebook_size):
            raise IndexError(f"codes outside [0, {self.codebook_size}): F.embedding of the reference raises here")
        z = torch.empty(B, self.latent_dim, T, device=dev)
        zp = torch.empty(B, n * self.codebook_dim, T, device=dev)
        with torch.cuda.device(dev):
            if fl is not None:
                _native.check(lib.escx_dac_from_codes_lengths(hd, ctypes.c_void_p(flat.data_ptr()), self._version(), ctypes.c_void_p(c.data_ptr()), B, n, T,
                                                              (ctypes.c_int32 * B)(*fl), None if counts is None else (ctypes.c_int32 * B)(*counts),
                                                              ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(zp.data_ptr()), stream))
            elif counts is None:
                _native.check(lib.escx_dac_from_codes(hd, ctypes.c_void_p(flat.data_ptr()), self._version(), ctypes.c_void_p(c.data_ptr()), B, n, T,
                                                      ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(zp.data_ptr()), stream))
            else:
                _native.check(lib.escx_dac_from_codes_ex(hd, ctypes.c_void_p(flat.data_ptr()), self._version(), ctypes.c_void_p(c.data_ptr()), B, n, T,
                                                         (ctypes.c_int32 * B)(*counts), ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(zp.data_ptr()), stream))
        return z, zp, codes

    # ---- the stand-alone quantiser (include/escx.h escx_dac_quantize and its neighbours) ----------------------------------
    def _quantizer_named(self):
        return [(k, p) for k, p in self.named_parameters() if k.startswith("quantizer.")]

    def _quantizer_trains(self) -> bool:
        return (self._encode_trainable in ("quantizer", "both") and torch.is_grad_enabled()
                and any(p.requires_grad for _, p in self._quantizer_named()))

    def _quantize_call(self, z: torch.Tensor, n: int, counts: Optional[List[int]], fl: Optional[List[int]]):
        """One escx_dac_quantize / _ex / _lengths call on a checked z: (z_q, codes, latents, losses (2,))."""
        lib, hd, flat, dev, stream = self._ctx(z, "z")
        B, _, T = z.shape
        zc = z.to(torch.float32).contiguous()
        zq = torch.empty(B, self.latent_dim, T, device=dev)
        codes = torch.empty(B, n, T, dtype=torch.int64, device=dev)
        latents = torch.empty(B, n * self.codebook_dim, T, device=dev)
        losses = torch.empty(2, device=dev)
        cn = (ctypes.c_int32 * B)(*counts) if counts is not None else None
        head = (hd, ctypes.c_void_p(flat.data_ptr()), self._version(), ctypes.c_void_p(zc.data_ptr()), B, T)
        outs = (ctypes.c_void_p(zq.data_ptr()), ctypes.c_void_p(codes.data_ptr()), ctypes.c_void_p(latents.data_ptr()), ctypes.c_void_p(losses.data_ptr()), stream)
        with torch.cuda.device(dev):
            if fl is not None:
                _native.check(lib.escx_dac_quantize_lengths(*head, (ctypes.c_int32 * B)(*fl), n, cn, *outs))
            elif counts is not None:
                _native.check(lib.escx_dac_quantize_ex(*head, n, cn, *outs))
            else:
                _native.check(lib.escx_dac_quantize(*head, n, *outs))
        return zq, codes, latents, losses

    def _quantize(self, z: torch.Tensor, n_quantizers: Union[int, Sequence[int], torch.Tensor] = None, frame_lengths=None):
        """ResidualVectorQuantize.forward in eval mode (quantize.py:127-198) on a latent the caller brings; `model.quantizer(z, n_quantizers)` is this
        method: (z_q (B, D, T), codes (B, n, T) int64, latents (B, n d, T), commitment_loss, codebook_loss).  z is (B, latent_dim, T); the values
        are the ones the quantiser inside encode computes from the same map, in every precision mode and whatever `padding` says.  n_quantizers
        is None, an int (above n_codebooks means n_codebooks) or one count per clip, with encode's semantics and fillers (codes -1, latents 0).
        frame_lengths (one frame count in [1, T] per clip; not part of the reference's surface) has decode's semantics: nothing at or past a clip's
        length is read, z_q and latents are 0 and codes -1 there, clip b is bitwise the call on z[b:b+1, :, :frame_lengths[b]] alone and the
        losses are the mean of the single-clip calls' losses; no gradients with it.

        When gradients are enabled and z requires one, z_q, latents and commitment_loss carry the gradient of the reference's eval-mode autograd:
        the straight-through estimator per stage and the commitment term against the detached codebook vector (quantize.py:58-70;
        `_QuantizeGrad`); codes and codebook_loss carry none.  After set_encode_trainable("quantizer" | "both") every quantiser parameter that
        requires a gradient gets one too - in_proj / out_proj bias, weight_g, weight_v and, through codebook_loss, the codebooks - and a stage
        no clip runs gets None (`_QuantizeParamGrad`); z.grad is bitwise the frozen path's."""
        if self.training:
            raise NotImplementedError("esc.baselines.DAC is inference only: call .eval() (DAC training is not implemented)")
        if not isinstance(z, torch.Tensor) or z.dim() != 3 or z.shape[1] != self.latent_dim or z.shape[0] < 1 or z.shape[2] < 1:
            raise ValueError(f"z must be (B, {self.latent_dim}, T) with B, T >= 1, got {tuple(getattr(z, 'shape', ()))}")
        B, _, T = z.shape
        counts = self._clip_counts(n_quantizers, B) if self._is_per_clip(n_quantizers) else None
        n = self._n_quantizers(n_quantizers) if counts is None else max(counts)
        fl = None if frame_lengths is None else self._clip_lengths(frame_lengths, B, T, "frame_lengths")
        _check_device(z, "z")
        wants, trains = torch.is_grad_enabled() and z.requires_grad, self._quantizer_trains()
        if fl is not None and (wants or trains):
            raise NotImplementedError("quantizer with frame_lengths is not implemented on the gradient paths (a z that requires grad, or "
                                      "set_encode_trainable with a quantiser parameter that requires grad): call it under torch.no_grad() or "
                                      "differentiate clip by clip")
        if trains:
            named = self._quantizer_named()
            return _QuantizeParamGrad.apply(z, self, n, counts, tuple(k for k, _ in named), *[p for _, p in named])
        if wants:
            return _QuantizeGrad.apply(z, self, n, counts)
        with torch.no_grad():
            zq, codes, latents, losses = self._quantize_call(z, n, counts, fl)
        return zq, codes, latents, losses[0], losses[1]

    @torch.no_grad()
    def _from_latents(self, latents: torch.Tensor, n_quantizers: Union[int, Sequence[int], torch.Tensor] = None, frame_lengths=None):
        """ResidualVectorQuantize.from_latents (quantize.py:222-255): per-codebook latents (B, C, T) that something else predicted ->
        (z_q (B, D, T), z_p (B, n d, T), codes (B, n, T) int64); `model.quantizer.from_latents` is this method.  n = min(C // codebook_dim,
        n_codebooks); trailing channels that fill no codebook are ignored and C < codebook_dim raises ValueError.  Every stage searches its own d
        channels independently (VectorQuantize.decode_latents, quantize.py:78-94), so the codes are bitwise the ones quantizer(z) emits for the
        same latents, and (z_q, z_p) are bitwise from_codes(codes)[:2].  n_quantizers (an int or one count per clip, each at most n) and
        frame_lengths are this port's extensions, as on from_codes: a stage slot past a clip's count holds code -1 and z_p 0, and the rows at or
        past a clip's frames hold 0 / -1 and are not read.  The search has no gradient in the reference and none here: the outputs never carry a
        grad_fn, and parameter gradients through from_latents are not built (train the quantiser through quantizer(z) or encode)."""
        if self.training:
            raise NotImplementedError("esc.baselines.DAC is inference only: call .eval() (DAC training is not implemented)")
        if not isinstance(latents, torch.Tensor) or latents.dim() != 3 or latents.shape[0] < 1 or latents.shape[2] < 1:
            raise ValueError(f"latents must be (B, C, T) with B, T >= 1, got {tuple(getattr(latents, 'shape', ()))}")
        B, C, T = latents.shape
        if C < self.codebook_dim:
            raise ValueError(f"latents of {C} channels hold no codebook of {self.codebook_dim} dimensions")
        n = min(C // self.codebook_dim, self.n_codebooks)
        counts = None
        if n_quantizers is not None:
            counts = self._clip_counts(n_quantizers if self._is_per_clip(n_quantizers) else [n_quantizers] * B, B)
            if max(counts) > n:
                raise ValueError(f"per-clip n_quantizers up to {max(counts)} for latents of {n} codebooks")
        fl = None if frame_lengths is None else self._clip_lengths(frame_lengths, B, T, "frame_lengths")
        lib, hd, flat, dev, stream = self._ctx(latents, "latents")
        lc = latents.to(torch.float32).contiguous()
        z = torch.empty(B, self.latent_dim, T, device=dev)
        zp = torch.empty(B, n * self.codebook_dim, T, device=dev)
        codes = torch.empty(B, n, T, dtype=torch.int64, device=dev)
        cn = (ctypes.c_int32 * B)(*counts) if counts is not None else None
        head = (hd, ctypes.c_void_p(flat.data_ptr()), self._version(), ctypes.c_void_p(lc.data_ptr()), B, C, T)
        outs = (ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(zp.data_ptr()), ctypes.c_void_p(codes.data_ptr()), stream)
        with torch.cuda.device(dev):
            if fl is not None:
                _native.check(lib.escx_dac_from_latents_lengths(*head, (ctypes.c_int32 * B)(*fl), cn, *outs))
            elif counts is not None:
                _native.check(lib.escx_dac_from_latents_ex(*head, cn, *outs))
            else:
                _native.check(lib.escx_dac_from_latents(*head, *outs))
        return z, zp, codes

    def forward(self, audio_data: torch.Tensor, sample_rate: int = None, n_quantizers: Union[int, Sequence[int], torch.Tensor] = None, lengths=None):
        """dac.py:268-323 in eval mode: right-pad to a multiple of the hop, encode, decode, trim the audio to the input length.  n_quantizers
        may be one count per clip, as in encode.  lengths (one sample count in [1, L] per clip): every clip goes through the reference's
        preprocess on its own - the samples from lengths[b] up to the next multiple of the hop are staged as zeros, not read - then encode and
        decode; out["audio"][b, :, :lengths[b]] is bitwise forward(audio_data[b:b+1, :, :lengths[b]])["audio"] and 0 from there on, and the
        dict gains "frame_lengths" (1-D int64 on the CPU: the frames of every clip in z, codes and latents)."""
        if self.training:
            raise NotImplementedError("esc.baselines.DAC is inference only: call .eval() (DAC training is not implemented)")
        if lengths is not None:
            hop = self.hop_length
            self._refuse_lengths("forward with lengths",
                                 (torch.is_grad_enabled() and isinstance(audio_data, torch.Tensor) and audio_data.requires_grad) or self._decoder_trains()
                                 or self._encoder_trains())
            lens, frames = self._check_encode_lengths(audio_data, lengths, hop)
            if self._is_per_clip(n_quantizers):
                n_quantizers = self._clip_counts(n_quantizers, audio_data.shape[0])
            if sample_rate is not None and sample_rate != self.sample_rate:
                raise AssertionError(f"sample_rate {sample_rate} != the model's {self.sample_rate}")
            _check_device(audio_data, "audio_data")
            z, codes, latents, cm, cb = self._encode_lengths(audio_data, lens, frames, n_quantizers, hop)
            audio = self._decode_lengths(z, frames, lens)
            return {"audio": audio[..., :audio_data.shape[-1]], "z": z, "codes": codes, "latents": latents, "vq/commitment_loss": cm,
                    "vq/codebook_loss": cb, "frame_lengths": torch.tensor(frames, dtype=torch.int64)}
        if self._is_per_clip(n_quantizers):
            n_quantizers = self._clip_counts(n_quantizers, audio_data.shape[0])
        _check_device(audio_data, "audio_data")
        length = audio_data.shape[-1]
        x = self.preprocess(audio_data, sample_rate)
        z, codes, latents, cm, cb = self.encode(x, n_quantizers)
        audio = self.decode(z)
        return {"audio": audio[..., :length], "z": z, "codes": codes, "latents": latents, "vq/commitment_loss": cm, "vq/codebook_loss": cb}

    # ---- CodecMixin.compress / decompress (base.py:125-294) ---------------------------------------------------------------------------------
    def _max_map(self, n: int, decoder: bool) -> int:
        """Elements of the largest channels-last feature map one clip of n samples (decoder: n frames) needs, an upper bound of what
        csrc/dac.hip sizes its scratch by (lengths only shrink inside a block, so the padded lengths bound the unpadded ones)."""
        cp = lambda c: (c + 3) // 4 * 4                                                          # noqa: E731
        if decoder:
            t, c, m = n, self.decoder_dim, n * max(cp(self.latent_dim), cp(self.decoder_dim))
            for s in self.decoder_rates:
                t, c = (t + 1) * s, c // 2
                m = max(m, t * cp(c))
            return m
        t, c, m = n, self.encoder_dim, n * max(4, cp(self.encoder_dim))
        for s in self.encoder_rates:
            t, c = t // s + 1, 2 * c
            m = max(m, t * cp(c))
        return max(m, t * cp(self.latent_dim))

    def chunk_schedule(self, n_signal: int, win_duration: Optional[float] = 1.0):
        """The schedule of base.py:182-214 for a signal of n_signal samples at the model's rate, reproduced as it stands (n_samples - hop is not
        2 * delay): {"padding", "n_samples", "hop", "starts", "chunk_length", "delay"}.  `padding` True is the unchunked pass (one window of the
        whole signal, taken when n_signal / sample_rate <= win_duration); otherwise window c covers [starts[c], starts[c] + n_samples) of the
        signal zero-padded by `delay` on both sides and chunk_length is the frames every window encodes to."""
        nt = int(n_signal)
        if nt < 1:
            raise ValueError("an empty signal")
        if win_duration is None or nt / self.sample_rate <= win_duration:
            t = math.ceil(nt / self.hop_length) * self.hop_length                # preprocess, then the padded encoder's length formula
            for s in self.encoder_rates:
                t = max((t + 2 * math.ceil(s / 2) - 2 * s) // s + 1, 0)
            return {"padding": True, "n_samples": nt, "hop": nt, "starts": [0], "chunk_length": t, "delay": 0}
        n_samples = int(win_duration * self.sample_rate)
        n_samples = int(math.ceil(n_samples / self.hop_length) * self.hop_length)
        hop = self.get_output_length(n_samples)
        layers = self._conv_layers()
        n_enc = 2 + 7 * len(self.encoder_rates)
        frames = self._walk(n_samples, layers[:n_enc]) if n_samples >= 1 else 0
        if hop < 1 or frames < 1 or self._walk(frames, layers[n_enc:]) != hop:
            raise ValueError(f"win_duration {win_duration} s is {n_samples} samples: below the receptive field of the unpadded model "
                             f"(get_output_length gives {hop})")
        return {"padding": False, "n_samples": n_samples, "hop": hop, "starts": list(range(0, nt, hop)), "chunk_length": frames,
                "delay": self.get_delay()}

    @_no_grad_frozen("compress")
    def compress(self, audio: torch.Tensor, sample_rate: int = None, win_duration: Optional[float] = 1.0, n_quantizers: int = None, input_db=None,
                 chunks_per_pass: int = None, lengths=None) -> DACFile:
        """CodecMixin.compress (base.py:125-233) for a tensor `audio` of shape (nt,), (channels, nt) or (batch, channels, nt) on the device.
        A signal of at most win_duration seconds is one padded pass.  A longer one is encoded with `padding` off in windows of
        n_samples = ceil(int(win_duration * sr) / hop_length) * hop_length samples that start every get_output_length(n_samples) samples of the
        signal zero-padded by `delay` on both sides.  The windows are staged on the device straight from the signal
        (include/escx.h escx_dac_encode_chunks) and run as one batch - the reference runs them one by one - or in passes of chunks_per_pass
        windows; the default takes all of them, split only where a pass would exceed the kernels' 2^32-element feature maps.  The codes do not
        depend on chunks_per_pass.  `padding` is back at its previous value on return, also after an error.

        Out of scope, because they are audiotools.AudioSignal's work and audiotools is not a dependency: resampling (a sample_rate other than
        the model's raises ValueError), loudness measurement and normalisation (input_db is stored in the file as given and not applied) and
        peak limiting.  The caller hands in the signal the reference would encode after those steps."""
        if lengths is not None:
            raise NotImplementedError("compress takes no per-clip lengths: a DACFile holds one original_length for all its rows (compress signals of "
                                      "different lengths one by one, or tokenise them with encode and lengths)")
        if self.training:
            raise NotImplementedError("esc.baselines.DAC is inference only: call .eval() (DAC training is not implemented)")
        if sample_rate is not None and sample_rate != self.sample_rate:
            raise ValueError(f"sample_rate {sample_rate} != the model's {self.sample_rate}: resampling is out of scope (audiotools)")
        if audio.dim() not in (1, 2, 3):
            raise ValueError(f"audio must be (nt,), (channels, nt) or (batch, channels, nt), got {tuple(audio.shape)}")
        if chunks_per_pass is not None and int(chunks_per_pass) < 1:
            raise ValueError(f"chunks_per_pass must be at least 1, got {chunks_per_pass}")
        x = audio.reshape((1,) * (3 - audio.dim()) + tuple(audio.shape))
        nb, nac, nt = x.shape
        rows = nb * nac
        n = self._n_quantizers(n_quantizers)
        previous = self.padding
        try:
            sch = self.chunk_schedule(nt, win_duration)
            self.padding = sch["padding"]
            x = x.reshape(rows, 1, nt)
            if sch["padding"]:
                codes = self.encode(self.preprocess(x, self.sample_rate), n)[1]
            else:
                codes = self._encode_chunks(x, sch, n, chunks_per_pass)
            return DACFile(codes=codes, chunk_length=sch["chunk_length"], original_length=nt, input_db=input_db, channels=nac,
                           sample_rate=self.sample_rate, padding=sch["padding"], dac_version=SUPPORTED_VERSIONS[-1])
        finally:
            self.padding = previous

    def _encode_chunks(self, x: torch.Tensor, sch: dict, n: int, chunks_per_pass):
        """codes (rows, n, n_chunks * chunk_length) of every window of the schedule, in passes of one batch each."""
        lib, hd, flat, dev, stream = self._ctx(x, "audio")
        rows, _, nt = x.shape
        n_samples, hop, T, n_chunks = sch["n_samples"], sch["hop"], sch["chunk_length"], len(sch["starts"])
        per = _MAP_LIMIT // (self._max_map(n_samples, False) * rows)
        if per < 1:
            raise NotImplementedError(f"{rows} rows of {n_samples}-sample windows: one chunk per row is above the 2^32-element feature maps")
        per = min(n_chunks, per if chunks_per_pass is None else min(per, int(chunks_per_pass)))
        if lib.escx_dac_num_frames(hd, n_samples) != T:
            raise RuntimeError(f"libescx encodes a {n_samples}-sample window to {lib.escx_dac_num_frames(hd, n_samples)} frames, the host to {T}")
        sig = x.to(torch.float32).contiguous()
        out = []
        for c0 in range(0, n_chunks, per):
            nc = min(per, n_chunks - c0)
            B = rows * nc
            z = torch.empty(B, self.latent_dim, T, device=dev)
            codes = torch.empty(B, n, T, dtype=torch.int64, device=dev)
            latents = torch.empty(B, n * self.codebook_dim, T, device=dev)
            losses = torch.empty(2, device=dev)
            with torch.cuda.device(dev):
                _native.check(lib.escx_dac_encode_chunks(hd, ctypes.c_void_p(flat.data_ptr()), self._version(), ctypes.c_void_p(sig.data_ptr()), rows, nt, nc,
                                                         n_samples, hop, sch["delay"] - c0 * hop, n, ctypes.c_void_p(z.data_ptr()),
                                                         ctypes.c_void_p(codes.data_ptr()), ctypes.c_void_p(latents.data_ptr()),
                                                         ctypes.c_void_p(losses.data_ptr()), stream))
            out.append(codes.reshape(rows, nc, n, T).permute(0, 2, 1, 3).reshape(rows, n, nc * T))
        return torch.cat(out, dim=-1)

    @torch.no_grad()
    def decompress(self, obj: Union[str, Path, DACFile], chunks_per_pass: int = None) -> torch.Tensor:
        """CodecMixin.decompress (base.py:235-294): the signal (batch, channels, original_length) of a DACFile or of a .dac file.  `padding` is
        taken from the file; the codes are decoded chunk_length frames at a time through quantizer.from_codes and decode, all chunks as one
        batch (or chunks_per_pass at a time, split as in compress), a shorter last chunk in a pass of its own, and the result is trimmed to
        original_length.  With the padding off each chunk decodes to exactly the hop of compress, so the chunks' outputs in batch order are the
        concatenated signal.  One deliberate departure: the unchunked path decodes fewer samples than it was given (320 T - 8 for rates
        [8, 5, 4, 2]); the reference's final reshape fails there, this method right-pads with zeros.  Loudness restoration and resampling are out
        of scope as in compress: a file of another sample rate raises ValueError.  `padding` is restored on return."""
        if self.training:
            raise NotImplementedError("esc.baselines.DAC is inference only: call .eval() (DAC training is not implemented)")
        if isinstance(obj, (str, Path)):
            obj = DACFile.load(obj)
        if int(obj.sample_rate) != self.sample_rate:
            raise ValueError(f"the file's sample_rate {obj.sample_rate} != the model's {self.sample_rate}: resampling is out of scope (audiotools)")
        if chunks_per_pass is not None and int(chunks_per_pass) < 1:
            raise ValueError(f"chunks_per_pass must be at least 1, got {chunks_per_pass}")
        codes, cl, length = obj.codes, int(obj.chunk_length), int(obj.original_length)
        if codes.dim() != 3 or cl < 1 or codes.shape[-1] < 1:
            raise ValueError(f"codes must be (rows, n, frames) with a positive chunk_length, got {tuple(codes.shape)} and {cl}")
        dev = codes.device if codes.is_cuda else self.device
        _check_device(torch.empty(0, device=dev), "the model")
        codes = codes.to(device=dev, dtype=torch.int64)
        rows, n, total = codes.shape
        previous = self.padding
        try:
            self.padding = bool(obj.padding)
            full = total // cl
            per = max(1, _MAP_LIMIT // (self._max_map(cl, True) * rows))
            per = per if chunks_per_pass is None else min(per, int(chunks_per_pass))
            recons = []
            for c0 in range(0, full, per):
                nc = min(per, full - c0)
                c = codes[..., c0 * cl:(c0 + nc) * cl].reshape(rows, n, nc, cl).permute(0, 2, 1, 3).reshape(rows * nc, n, cl)
                r = self.decode(self._from_codes(c)[0])
                assert r.shape[-1] == self.output_samples(cl)
                recons.append(r.reshape(rows, 1, nc * r.shape[-1]))
            if total % cl:
                recons.append(self.decode(self._from_codes(codes[..., full * cl:].contiguous())[0]))
            out = torch.cat(recons, dim=-1)[..., :length]
            if out.shape[-1] < length:
                out = nn.functional.pad(out, (0, length - out.shape[-1]))
            return out.reshape(-1, int(obj.channels), length)
        finally:
            self.padding = previous

    @classmethod
    def load(cls, path, map_location="cpu", strict: bool = True):
        """A checkpoint in the layout audiotools' BaseModel.save_to_folder writes (the reference trainer's, scripts/train_customize_no_adv.py:324):
        a torch.save'd dict with "state_dict" and "metadata": {"kwargs": constructor keywords}.  That layout is assumed from the reference's
        code, not checked against a real file."""
        ck = torch.load(path, map_location=map_location, weights_only=False)
        kwargs = dict(ck["metadata"]["kwargs"])
        model = cls(**kwargs)
        model.load_state_dict(ck["state_dict"], strict=strict)
        model.metadata = ck["metadata"]
        return model


class _DecodeGrad(torch.autograd.Function):
    """DAC.decode with the latent gradient (include/escx.h escx_dac_decode_tape / escx_dac_decode_backward): the frozen decoder inside a larger
    autograd graph.  forward is the decode's own launch sequence with the maps the backward needs kept in a tape, a plain tensor saved on the
    graph, so any number of graphs may be alive at once; backward is first order only and runs in the arithmetic of set_grad_precision
    at the time it is called (fp32 MFMA by default, whatever set_precision says)."""

    @staticmethod
    def forward(ctx, z, model):
        lib, hd, flat, dev, stream, B, T, n_out = model._decode_args(z)
        if not model._padding:
            raise NotImplementedError("the latent gradient of DAC.decode is implemented with padding on (the chunked path needs no gradients)")
        zc = z.detach().to(torch.float32).contiguous()
        floats = int(lib.escx_dac_decode_tape_floats(hd, B, T))
        if floats < 0:
            _native.check(floats)
        if floats < 1:
            raise RuntimeError(f"libescx gives no tape for a decode of {B} x {T} frames")
        tape = torch.empty(floats, dtype=torch.float32, device=dev)
        out = torch.empty(B, 1, n_out, device=dev)
        version = model._version()
        with torch.cuda.device(dev):
            _native.check(lib.escx_dac_decode_tape(hd, ctypes.c_void_p(flat.data_ptr()), version, ctypes.c_void_p(zc.data_ptr()), B, T,
                                                   ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(tape.data_ptr()), floats, stream))
        ctx.save_for_backward(tape)
        ctx.model, ctx.version, ctx.dims, ctx.z_dtype = model, version, (B, T), z.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_audio):
        model, (B, T) = ctx.model, ctx.dims
        tape, = ctx.saved_tensors
        if model._version() != ctx.version:
            raise RuntimeError("a parameter of the DAC module was changed in place between decode and its backward: the tape was made with the "
                               "earlier weights (decode again after changing parameters)")
        lib, hd, flat, dev, stream = model._ctx(tape, "the tape")
        g = d_audio.to(torch.float32).contiguous()
        d_z = torch.empty(B, model.latent_dim, T, device=dev)
        with torch.cuda.device(dev):
            _native.check(lib.escx_dac_decode_backward(hd, ctypes.c_void_p(flat.data_ptr()), ctx.version, ctypes.c_void_p(tape.data_ptr()), tape.numel(),
                                                       ctypes.c_void_p(g.data_ptr()), B, T, ctypes.c_void_p(d_z.data_ptr()), stream))
        return d_z.to(ctx.z_dtype), None


class _DecodeParamGrad(torch.autograd.Function):
    """DAC.decode with the gradients of the decoder's parameters (include/escx.h escx_dac_decode_backward_params), for fine-tuning a decoder on
    frozen codes or latents after set_trainable("decoder").  forward is `_DecodeGrad`'s: the decode's own launch sequence with its maps kept in a
    tape on the graph.  backward returns the gradient of every decoder parameter that requires one, and of z if it requires one (bitwise
    `_DecodeGrad`'s); autograd accumulates them into p.grad.  First order only; no atomics.  The input gradients run in
    set_grad_precision's arithmetic at the time backward is called, the weight-gradient contractions in set_param_grad_precision's (fp32 MFMA
    by default)."""

    @staticmethod
    def forward(ctx, z, model, *params):
        lib, hd, flat, dev, stream, B, T, n_out = model._decode_args(z)
        if not model._padding:
            raise NotImplementedError("the parameter gradients of DAC.decode are implemented with padding on (the chunked path needs no gradients)")
        zc = z.detach().to(torch.float32).contiguous()
        floats = int(lib.escx_dac_decode_tape_floats(hd, B, T))
        if floats < 0:
            _native.check(floats)
        if floats < 1:
            raise RuntimeError(f"libescx gives no tape for a decode of {B} x {T} frames")
        tape = torch.empty(floats, dtype=torch.float32, device=dev)
        out = torch.empty(B, 1, n_out, device=dev)
        version = model._version()
        with torch.cuda.device(dev):
            _native.check(lib.escx_dac_decode_tape(hd, ctypes.c_void_p(flat.data_ptr()), version, ctypes.c_void_p(zc.data_ptr()), B, T,
                                                   ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(tape.data_ptr()), floats, stream))
        ctx.save_for_backward(tape, zc)
        ctx.model, ctx.version, ctx.dims, ctx.z_dtype = model, version, (B, T), z.dtype
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_audio):
        model, (B, T) = ctx.model, ctx.dims
        tape, zc = ctx.saved_tensors
        if model._version() != ctx.version:
            raise RuntimeError("a parameter of the DAC module was changed in place between decode and its backward: the tape was made with the "
                               "earlier weights (decode again after changing parameters)")
        lib, hd, flat, dev, stream = model._ctx(tape, "the tape")
        g = d_audio.to(torch.float32).contiguous()
        d_z = torch.empty(B, model.latent_dim, T, device=dev) if ctx.needs_input_grad[0] else None
        grad = torch.empty_like(flat)                        # only the decoder's slots are written, and only they are read below
        with torch.cuda.device(dev):
            _native.check(lib.escx_dac_decode_backward_params(hd, ctypes.c_void_p(flat.data_ptr()), ctx.version, ctypes.c_void_p(tape.data_ptr()), tape.numel(),
                                                              ctypes.c_void_p(zc.data_ptr()), ctypes.c_void_p(g.data_ptr()), B, T,
                                                              None if d_z is None else ctypes.c_void_p(d_z.data_ptr()), ctypes.c_void_p(grad.data_ptr()),
                                                              stream))
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        slots = [(off, n) for key, off, n in model._flat[idx]["layout"] if key.startswith("decoder.")]
        params = list(model.decoder_parameters())
        # views of the one buffer: the slots are disjoint, so the p.grad that autograd makes of them never alias each other
        grads = [grad[off:off + n].view(p.shape) if need else None for (off, n), p, need in zip(slots, params, ctx.needs_input_grad[2:])]
        return (None if d_z is None else d_z.to(ctx.z_dtype), None, *grads)


class _EncodeGrad(torch.autograd.Function):
    """DAC.encode with the audio gradient (include/escx.h escx_dac_encode_tape / escx_dac_encode_backward): the reference's eval-mode autograd
    through the encoder and the quantiser's straight-through estimator (quantize.py:58-70, 173-198).  z, latents and the commitment loss are
    differentiable; the codes are integers and the codebook loss detaches z_e.  forward is the encode's own launch sequence with the maps, latents,
    codes and stage counts the backward needs kept in a tape, a plain tensor saved on the graph; backward is first order only and runs on the
    The encoder layers' input gradients run in set_grad_precision's arithmetic at the time backward is called (fp32 MFMA by default), the
    quantiser's backward on the fp32 VALU.  counts: one stage count per clip, or None for n stages everywhere."""

    @staticmethod
    def forward(ctx, audio_data, model, n, counts):
        lib, hd, flat, dev, stream = model._ctx(audio_data, "audio_data")
        if not model._padding:
            raise NotImplementedError("the audio gradient of DAC.encode is implemented with padding on (the chunked path needs no gradients)")
        B, L, T = model._audio_shape(audio_data)
        x = audio_data.detach().to(torch.float32).contiguous()
        floats = int(lib.escx_dac_encode_tape_floats(hd, B, L, n))
        if floats < 0:
            _native.check(floats)
        if floats < 1:
            raise RuntimeError(f"libescx gives no tape for an encode of {B} x {L} samples")
        tape = torch.empty(floats, dtype=torch.float32, device=dev)
        z = torch.empty(B, model.latent_dim, T, device=dev)
        codes = torch.empty(B, n, T, dtype=torch.int64, device=dev)
        latents = torch.empty(B, n * model.codebook_dim, T, device=dev)
        losses = torch.empty(2, device=dev)
        version = model._version()
        cn = (ctypes.c_int32 * B)(*counts) if counts is not None else None
        with torch.cuda.device(dev):
            _native.check(lib.escx_dac_encode_tape(hd, ctypes.c_void_p(flat.data_ptr()), version, ctypes.c_void_p(x.data_ptr()), B, L, n, cn,
                                                   ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(codes.data_ptr()), ctypes.c_void_p(latents.data_ptr()),
                                                   ctypes.c_void_p(losses.data_ptr()), ctypes.c_void_p(tape.data_ptr()), floats, stream))
        cm, cb = losses[0].clone(), losses[1].clone()
        ctx.save_for_backward(tape)
        ctx.model, ctx.version, ctx.dims, ctx.x_dtype = model, version, (B, L), audio_data.dtype
        ctx.mark_non_differentiable(codes, cb)
        ctx.set_materialize_grads(False)                     # an output the loss does not use hands None to backward: a NULL cotangent, not a map of zeros
        return z, codes, latents, cm, cb

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_z, _d_codes, d_latents, d_cm, _d_cb):
        model, (B, L) = ctx.model, ctx.dims
        tape, = ctx.saved_tensors
        if model._version() != ctx.version:
            raise RuntimeError("a parameter of the DAC module was changed in place between encode and its backward: the tape was made with the "
                               "earlier weights (encode again after changing parameters)")
        lib, hd, flat, dev, stream = model._ctx(tape, "the tape")
        gs = [None if g is None else g.to(device=dev, dtype=torch.float32).contiguous() for g in (d_z, d_latents, d_cm)]
        ptr = [None if g is None else ctypes.c_void_p(g.data_ptr()) for g in gs]
        d_audio = torch.empty(B, 1, L, device=dev)
        with torch.cuda.device(dev):
            _native.check(lib.escx_dac_encode_backward(hd, ctypes.c_void_p(flat.data_ptr()), ctx.version, ctypes.c_void_p(tape.data_ptr()), tape.numel(),
                                                       ptr[0], ptr[1], ptr[2], B, L, ctypes.c_void_p(d_audio.data_ptr()), stream))
        return d_audio.to(ctx.x_dtype), None, None, None


class _EncodeParamGrad(torch.autograd.Function):
    """DAC.encode with the gradients of the encoder's and / or the quantiser's parameters (include/escx.h escx_dac_encode_backward_params), for
    fine-tuning after set_encode_trainable.  forward is `_EncodeGrad`'s: the encode's own launch sequence with its maps kept in a tape on the
    graph; the audio is saved next to it (the tape does not hold it).  backward returns the gradient of every parameter of the chosen part that
    requires one and whose quantiser stage the call ran, and of the audio if it requires one (bitwise `_EncodeGrad`'s); autograd accumulates
    them into p.grad.  With the quantiser chosen the codebook loss carries the codebooks' gradient.  First order only; no atomics.  The input
    gradients run in set_grad_precision's arithmetic at the time backward is called, the encoder's weight-gradient contractions in
    set_param_grad_precision's, the quantiser's kernels in fp32.  keys: the names of `params`, in state_dict order."""

    @staticmethod
    def forward(ctx, audio_data, model, n, counts, keys, *params):
        lib, hd, flat, dev, stream = model._ctx(audio_data, "audio_data")
        if not model._padding:
            raise NotImplementedError("the parameter gradients of DAC.encode are implemented with padding on (the chunked path needs no gradients)")
        B, L, T = model._audio_shape(audio_data)
        x = audio_data.detach().to(torch.float32).contiguous()
        floats = int(lib.escx_dac_encode_tape_floats(hd, B, L, n))
        if floats < 0:
            _native.check(floats)
        if floats < 1:
            raise RuntimeError(f"libescx gives no tape for an encode of {B} x {L} samples")
        tape = torch.empty(floats, dtype=torch.float32, device=dev)
        z = torch.empty(B, model.latent_dim, T, device=dev)
        codes = torch.empty(B, n, T, dtype=torch.int64, device=dev)
        latents = torch.empty(B, n * model.codebook_dim, T, device=dev)
        losses = torch.empty(2, device=dev)
        version = model._version()
        cn = (ctypes.c_int32 * B)(*counts) if counts is not None else None
        with torch.cuda.device(dev):
            _native.check(lib.escx_dac_encode_tape(hd, ctypes.c_void_p(flat.data_ptr()), version, ctypes.c_void_p(x.data_ptr()), B, L, n, cn,
                                                   ctypes.c_void_p(z.data_ptr()), ctypes.c_void_p(codes.data_ptr()), ctypes.c_void_p(latents.data_ptr()),
                                                   ctypes.c_void_p(losses.data_ptr()), ctypes.c_void_p(tape.data_ptr()), floats, stream))
        cm, cb = losses[0].clone(), losses[1].clone()
        ctx.save_for_backward(tape, x)
        ctx.model, ctx.version, ctx.dims, ctx.x_dtype = model, version, (B, L), audio_data.dtype
        ctx.keys, ctx.stages, ctx.parts = keys, n, _ENCODE_PARTS[model._encode_trainable]
        if ctx.parts & 2:
            ctx.mark_non_differentiable(codes)               # the codebook loss is differentiable in the codebooks
        else:
            ctx.mark_non_differentiable(codes, cb)
        ctx.set_materialize_grads(False)                     # an output the loss does not use hands None to backward: a NULL cotangent, not a map of zeros
        return z, codes, latents, cm, cb

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_z, _d_codes, d_latents, d_cm, d_cb):
        model, (B, L) = ctx.model, ctx.dims
        tape, x = ctx.saved_tensors
        if model._version() != ctx.version:
            raise RuntimeError("a parameter of the DAC module was changed in place between encode and its backward: the tape was made with the "
                               "earlier weights (encode again after changing parameters)")
        lib, hd, flat, dev, stream = model._ctx(tape, "the tape")
        gs = [None if g is None else g.to(device=dev, dtype=torch.float32).contiguous() for g in (d_z, d_latents, d_cm, d_cb if ctx.parts & 2 else None)]
        ptr = [None if g is None else ctypes.c_void_p(g.data_ptr()) for g in gs]
        d_audio = torch.empty(B, 1, L, device=dev) if ctx.needs_input_grad[0] else None
        grad = torch.empty_like(flat)                        # only the chosen part's slots are written, and only they are read below
        with torch.cuda.device(dev):
            _native.check(lib.escx_dac_encode_backward_params(hd, ctypes.c_void_p(flat.data_ptr()), ctx.version, ctypes.c_void_p(tape.data_ptr()), tape.numel(),
                                                              ctypes.c_void_p(x.data_ptr()), ptr[0], ptr[1], ptr[2], ptr[3], B, L, ctx.parts,
                                                              None if d_audio is None else ctypes.c_void_p(d_audio.data_ptr()), ctypes.c_void_p(grad.data_ptr()),
                                                              stream))
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        slots = {key: (off, cnt) for key, off, cnt in model._flat[idx]["layout"]}
        named = dict(model.named_parameters())
        grads = []
        for key, need in zip(ctx.keys, ctx.needs_input_grad[5:]):
            # a quantiser stage the call did not run is not on the reference's graph: None, not the zeros the library wrote
            unused = key.startswith("quantizer.quantizers.") and int(key.split(".")[2]) >= ctx.stages
            off, cnt = slots[key]
            # views of the one buffer: the slots are disjoint, so the p.grad that autograd makes of them never alias each other
            grads.append(grad[off:off + cnt].view(named[key].shape) if need and not unused else None)
        return (None if d_audio is None else d_audio.to(ctx.x_dtype), None, None, None, None, *grads)


def _quantize_forward(ctx, z, model, n, counts):
    """The forward both quantiser Functions share: escx_dac_quantize / _ex, with what the backward reads kept on ctx.  There is no tape: the
    backward's operands are the forward's own latents and codes, saved as they are."""
    zq, codes, latents, losses = model._quantize_call(z.detach(), n, counts, None)
    cm, cb = losses[0].clone(), losses[1].clone()
    ctx.model, ctx.version, ctx.counts, ctx.z_dtype = model, model._version(), counts, z.dtype
    ctx.set_materialize_grads(False)                         # an output the loss does not use hands None to backward: a NULL cotangent, not a map of zeros
    return zq, codes, latents, cm, cb


def _quantize_backward_args(ctx, latents, codes, cotangents):
    """(lib, hd, flat, dev, stream, B, T, n, clip_n, pointers of the cotangents) of a quantiser backward, after the parameter-version check."""
    model = ctx.model
    if model._version() != ctx.version:
        raise RuntimeError("a parameter of the DAC module was changed in place between quantizer(z) and its backward: the latents and codes were "
                           "made with the earlier weights (quantise again after changing parameters)")
    lib, hd, flat, dev, stream = model._ctx(latents, "the latents")
    B, n, T = codes.shape
    gs = [None if g is None else g.to(device=dev, dtype=torch.float32).contiguous() for g in cotangents]
    cn = (ctypes.c_int32 * B)(*ctx.counts) if ctx.counts is not None else None
    return lib, hd, flat, dev, stream, B, T, n, cn, gs, [None if g is None else ctypes.c_void_p(g.data_ptr()) for g in gs]


class _QuantizeGrad(torch.autograd.Function):
    """model.quantizer(z) with the latent gradient (include/escx.h escx_dac_quantize / escx_dac_quantize_backward): the reference's eval-mode
    autograd through the residual quantiser (quantize.py:58-70, 173-198).  z_q, latents and the commitment loss are differentiable; the codes are
    integers and the codebook loss detaches z_e.  backward is one launch of the encoder path's quantiser backward on the forward's own latents
    and codes, then the store into z's layout; first order only, fp32 VALU, no atomics.  counts: one stage count per clip, or None."""

    @staticmethod
    def forward(ctx, z, model, n, counts):
        zq, codes, latents, cm, cb = _quantize_forward(ctx, z, model, n, counts)
        ctx.save_for_backward(latents, codes)
        ctx.mark_non_differentiable(codes, cb)
        return zq, codes, latents, cm, cb

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_zq, _d_codes, d_latents, d_cm, _d_cb):
        latents, codes = ctx.saved_tensors
        lib, hd, flat, dev, stream, B, T, n, cn, _gs, ptr = _quantize_backward_args(ctx, latents, codes, (d_zq, d_latents, d_cm))
        d_z = torch.empty(B, ctx.model.latent_dim, T, device=dev)
        with torch.cuda.device(dev):
            _native.check(lib.escx_dac_quantize_backward(hd, ctypes.c_void_p(flat.data_ptr()), ctx.version, ctypes.c_void_p(latents.data_ptr()),
                                                         ctypes.c_void_p(codes.data_ptr()), B, T, n, cn, ptr[0], ptr[1], ptr[2],
                                                         ctypes.c_void_p(d_z.data_ptr()), stream))
        return d_z.to(ctx.z_dtype), None, None, None


class _QuantizeParamGrad(torch.autograd.Function):
    """model.quantizer(z) with the gradients of the quantiser's parameters (include/escx.h escx_dac_quantize_backward_params), after
    set_encode_trainable("quantizer" | "both"): `_EncodeParamGrad`'s quantiser block on the staged z.  backward returns the gradient of every
    quantiser parameter that requires one and whose stage the call ran, and of z if it requires one (bitwise `_QuantizeGrad`'s); the codebook
    loss carries the codebooks' gradient.  First order only; no atomics.  keys: the names of `params`, in state_dict order."""

    @staticmethod
    def forward(ctx, z, model, n, counts, keys, *params):
        zq, codes, latents, cm, cb = _quantize_forward(ctx, z, model, n, counts)
        ctx.save_for_backward(latents, codes, z.detach().to(torch.float32).contiguous())
        ctx.keys, ctx.stages = keys, n
        ctx.mark_non_differentiable(codes)                   # the codebook loss is differentiable in the codebooks
        return zq, codes, latents, cm, cb

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_zq, _d_codes, d_latents, d_cm, d_cb):
        latents, codes, zc = ctx.saved_tensors
        model = ctx.model
        lib, hd, flat, dev, stream, B, T, n, cn, _gs, ptr = _quantize_backward_args(ctx, latents, codes, (d_zq, d_latents, d_cm, d_cb))
        d_z = torch.empty(B, model.latent_dim, T, device=dev) if ctx.needs_input_grad[0] else None
        grad = torch.empty_like(flat)                        # only the quantiser's slots are written, and only they are read below
        with torch.cuda.device(dev):
            _native.check(lib.escx_dac_quantize_backward_params(hd, ctypes.c_void_p(flat.data_ptr()), ctx.version, ctypes.c_void_p(zc.data_ptr()),
                                                                ctypes.c_void_p(latents.data_ptr()), ctypes.c_void_p(codes.data_ptr()), B, T, n, cn,
                                                                ptr[0], ptr[1], ptr[2], ptr[3], None if d_z is None else ctypes.c_void_p(d_z.data_ptr()),
                                                                ctypes.c_void_p(grad.data_ptr()), stream))
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        slots = {key: (off, cnt) for key, off, cnt in model._flat[idx]["layout"]}
        named = dict(model.named_parameters())
        grads = []
        for key, need in zip(ctx.keys, ctx.needs_input_grad[5:]):
            # a stage the call did not run is not on the reference's graph: None, not the zeros the library wrote
            off, cnt = slots[key]
            grads.append(grad[off:off + cnt].view(named[key].shape) if need and int(key.split(".")[2]) < ctx.stages else None)
        return (None if d_z is None else d_z.to(ctx.z_dtype), None, None, None, None, *grads)
