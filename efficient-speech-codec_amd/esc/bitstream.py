"""Wire / disk format of ESC codes.

The reference just `torch.save`s the int64 tensor (scripts/compress.py:35), i.e. 64 bits per 10-bit code.  Each code
indexes a 1024-entry codebook, so the real payload is 10 bits: 6 streams x 3 groups x 50 frames/s x 10 b = 9000 b/s,
which is where "9 kbps" comes from (esc/models/base.py:70).  `pack_codes` produces exactly that payload (plus a
16-byte header), packed on the GPU.

A mixed-bitrate batch (per-clip stream counts, `ESC.encode(x, [S_0, S_1, ...])`) travels as `ESC2`: the ESC1 header with magic "ESC2"
and S = max(S_b), then one byte per clip with S_b, then only the transmitted codes - clip b's first S_b streams, clips in order - as one
10-bit stream of ceil(10 * sum(S_b) * G * T / 8) bytes.
"""
from __future__ import annotations

import ctypes
import struct
from typing import Tuple

import torch

MAGIC = b"ESC1"
MAGIC2 = b"ESC2"
HEADER_BYTES = 16                   # ESC2: + one byte per clip (its stream count)
BITS = 10          # bits per code on the wire: codebook_size <= 1024


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def pack_codes(codes: torch.Tensor, feat_shape: Tuple[int, int], codebook_size: int = 1024, num_streams=None) -> bytes:
    """(B, S, G, T) int64 device tensor -> bytes: header (magic, B, S, G, T as u16, H, W as u16) + 10-bit payload.
    The format carries 10 bits per code: a model with codebook_size > 1024 (or a code outside [0, 1024)) is refused
    instead of being silently masked.  With `num_streams` (per-clip counts, each in [1, S]) the blob is ESC2 and carries
    clip b's first num_streams[b] streams only."""
    from . import _native
    if num_streams is not None:
        return _pack_codes_streams(codes, feat_shape, codebook_size, num_streams)
    if not codes.is_cuda:
        raise RuntimeError("pack_codes expects the codes on the HIP device they were produced on")
    if codebook_size > (1 << BITS):
        raise ValueError(f"the ESC1 wire format carries {BITS}-bit codes; codebook_size={codebook_size} does not fit")
    if codes.dim() != 4:
        raise ValueError("codes must have shape (B, S, G, T)")
    if max(codes.shape) > 0xFFFF or max(int(feat_shape[0]), int(feat_shape[1])) > 0xFFFF:
        raise ValueError("a header field exceeds 16 bits")
    lib = _native.load()
    c = codes.to(torch.int64).contiguous()
    n = c.numel()
    if n and (int(c.min()) < 0 or int(c.max()) >= (1 << BITS)):
        raise ValueError(f"code index outside [0, {1 << BITS}): the wire format would corrupt it")
    out = torch.empty(5 * ((n + 3) // 4), dtype=torch.uint8, device=c.device)
    with torch.cuda.device(c.device):
        _native.check(lib.escx_codes_pack10(ctypes.c_void_p(c.data_ptr()), ctypes.c_void_p(out.data_ptr()), n, _stream(c.device)))
    B, S, G, T = c.shape
    return MAGIC + struct.pack("<6H", B, S, G, T, int(feat_shape[0]), int(feat_shape[1])) + out.cpu().numpy().tobytes()


def _ragged_bytes(n: int) -> int:
    return (BITS * n + 7) // 8


def _pack_codes_streams(codes: torch.Tensor, feat_shape, codebook_size: int, num_streams) -> bytes:
    from . import _native
    if not codes.is_cuda:
        raise RuntimeError("pack_codes expects the codes on the HIP device they were produced on")
    if codebook_size > (1 << BITS):
        raise ValueError(f"the ESC2 wire format carries {BITS}-bit codes; codebook_size={codebook_size} does not fit")
    if codes.dim() != 4:
        raise ValueError("codes must have shape (B, S, G, T)")
    B, S, G, T = codes.shape
    counts = [int(v) for v in (num_streams.tolist() if isinstance(num_streams, torch.Tensor) else num_streams)]
    if len(counts) != B or B == 0:
        raise ValueError(f"num_streams has {len(counts)} entries for {B} clips")
    if min(counts) < 1 or max(counts) > S or S > 0xFF:
        raise ValueError(f"per-clip stream counts must lie in [1, {S}]")
    if max(B, S, G, T) > 0xFFFF or max(int(feat_shape[0]), int(feat_shape[1])) > 0xFFFF:
        raise ValueError("a header field exceeds 16 bits")
    c = codes.to(torch.int64).contiguous()
    sent = c[torch.arange(S, device=c.device)[None, :] < torch.tensor(counts, device=c.device)[:, None]]
    if sent.numel() and (int(sent.min()) < 0 or int(sent.max()) >= (1 << BITS)):
        raise ValueError(f"code index outside [0, {1 << BITS}): the wire format would corrupt it")
    n = sum(counts) * G * T
    out = torch.empty(5 * ((n + 3) // 4), dtype=torch.uint8, device=c.device)
    lib = _native.load()
    with torch.cuda.device(c.device):
        _native.check(lib.escx_codes_pack10_streams(ctypes.c_void_p(c.data_ptr()), B, S, G * T, (ctypes.c_int32 * B)(*counts),
                                                    ctypes.c_void_p(out.data_ptr()), _stream(c.device)))
    head = MAGIC2 + struct.pack("<6H", B, S, G, T, int(feat_shape[0]), int(feat_shape[1])) + bytes(counts)
    return head + out[:_ragged_bytes(n)].cpu().numpy().tobytes()      # the packer's last group is zero-padded to 5 bytes: only whole bits are sent


def parse_header2(blob: bytes):
    """(B, S, G, T, H, W, counts, header_bytes, payload_bytes) of an ESC2 stream; raises ValueError on a truncated or inconsistent blob."""
    if len(blob) < HEADER_BYTES or blob[:4] != MAGIC2:
        raise ValueError("not an ESC2 code stream")
    B, S, G, T, H, W = struct.unpack("<6H", blob[4:HEADER_BYTES])
    if min(B, S, G, T, H, W) == 0:
        raise ValueError(f"corrupt ESC2 header: zero dimension in {(B, S, G, T, H, W)}")
    head = HEADER_BYTES + B
    if len(blob) < head:
        raise ValueError("truncated ESC2 stream: per-clip stream counts missing")
    counts = list(blob[HEADER_BYTES:head])
    if min(counts) < 1 or max(counts) > S:
        raise ValueError(f"corrupt ESC2 header: stream counts outside [1, {S}]")
    need = _ragged_bytes(sum(counts) * G * T)
    if len(blob) < head + need:
        raise ValueError(f"truncated ESC2 stream: header announces {need} payload bytes, {len(blob) - head} present")
    return B, S, G, T, H, W, counts, head, need


def parse_header(blob: bytes):
    """(B, S, G, T, H, W, payload_bytes) of an ESC1 stream; raises ValueError on a truncated or inconsistent blob."""
    if len(blob) < HEADER_BYTES or blob[:4] != MAGIC:
        raise ValueError("not an ESC code stream")
    B, S, G, T, H, W = struct.unpack("<6H", blob[4:HEADER_BYTES])
    if min(B, S, G, T, H, W) == 0:
        raise ValueError(f"corrupt ESC1 header: zero dimension in {(B, S, G, T, H, W)}")
    need = 5 * ((B * S * G * T + 3) // 4)
    if len(blob) < HEADER_BYTES + need:
        raise ValueError(f"truncated ESC1 stream: header announces {need} payload bytes, {len(blob) - HEADER_BYTES} present")
    return B, S, G, T, H, W, need


def unpack_codes(blob: bytes, device="cuda", model=None):
    """Inverse of pack_codes: -> (codes int64 (B,S,G,T) on `device`, feat_shape).  With `model` given, the header is
    checked against the model (group_size, max_streams, overlap) before anything is decoded.  An ESC2 blob returns
    (codes, feat_shape, num_streams): codes are -1 past each clip's count, num_streams is the list of per-clip counts."""
    from . import _native
    if blob[:4] == MAGIC2:
        return _unpack_codes_streams(blob, device, model)
    B, S, G, T, H, W, need = parse_header(blob)
    if model is not None:
        c = model.cfg
        if G != c["group_size"] or S > model._code_streams or T * c["overlap"] != W or c["codebook_size"] > (1 << BITS):     # RVQCodecs: num_rvqs
            raise ValueError(f"ESC1 header {(B, S, G, T, H, W)} does not match the model (group_size {c['group_size']}, "
                             f"max_streams {c['max_streams']}, overlap {c['overlap']})")
    n = B * S * G * T
    payload = torch.frombuffer(bytearray(blob[HEADER_BYTES:HEADER_BYTES + need]), dtype=torch.uint8).to(device)
    lib = _native.load()
    codes = torch.empty((B, S, G, T), dtype=torch.int64, device=payload.device)
    with torch.cuda.device(payload.device):
        _native.check(lib.escx_codes_unpack10(ctypes.c_void_p(payload.data_ptr()), ctypes.c_void_p(codes.data_ptr()), n, _stream(payload.device)))
    return codes, (H, W)


def payload_bits_per_second(num_streams: int, group_size: int = 3, frames_per_second: float = 50.0, bits: int = 10) -> float:
    return num_streams * group_size * frames_per_second * bits


def _unpack_codes_streams(blob: bytes, device, model):
    from . import _native
    B, S, G, T, H, W, counts, head, need = parse_header2(blob)
    if model is not None:
        c = model.cfg
        if G != c["group_size"] or S > model._code_streams or T * c["overlap"] != W or c["codebook_size"] > (1 << BITS):     # RVQCodecs: num_rvqs
            raise ValueError(f"ESC2 header {(B, S, G, T, H, W)} does not match the model (group_size {c['group_size']}, "
                             f"max_streams {c['max_streams']}, overlap {c['overlap']})")
    n = sum(counts) * G * T
    raw = bytearray(blob[head:head + need]) + bytearray(5 * ((n + 3) // 4) - need)      # back to whole 5-byte groups for the unpacker
    payload = torch.frombuffer(raw, dtype=torch.uint8).to(device)
    codes = torch.empty((B, S, G, T), dtype=torch.int64, device=payload.device)
    lib = _native.load()
    with torch.cuda.device(payload.device):
        _native.check(lib.escx_codes_unpack10_streams(ctypes.c_void_p(payload.data_ptr()), B, S, G * T, (ctypes.c_int32 * B)(*counts),
                                                      ctypes.c_void_p(codes.data_ptr()), _stream(payload.device)))
    return codes, (H, W), counts
