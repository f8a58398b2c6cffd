"""Mixed-bitrate batches: per-clip stream counts in ESC.encode / ESC.decode / ESC.forward (include/escx.h escx_*_streams), the ragged
ESC2 wire format and the padded codes on the sharded path.

Every clip of a mixed batch must get exactly what a uniform call at its own count returns: the codes of S streams are the first S of the
S = 6 codes, a clip's results do not depend on the batch it is processed in, and untransmitted streams pass through the decoder."""
import ctypes
import json
import os
import struct
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, synth_state
from gpu_util import PRECISIONS, build_models, code_report, rms

AUDIO_TOL = 1e-4            # the whole-path audio tolerance of tests/test_gpu_parity.py


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _counts(vals):
    return (ctypes.c_int32 * len(vals))(*vals)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------ host-side reference of the ESC2 format ----------------------
def ref_pack_esc2(codes, feat_shape, counts):
    """Reference packer: header, one count byte per clip, then clip b's first counts[b] streams as 10-bit little-endian codes."""
    B, S, G, T = codes.shape
    flat = np.concatenate([np.asarray(codes[b, :counts[b]]).reshape(-1) for b in range(B)]).astype(np.int64)
    acc, nbits, out = 0, 0, bytearray()
    for v in flat:
        acc |= int(v) << nbits
        nbits += 10
        while nbits >= 8:
            out.append(acc & 0xFF); acc >>= 8; nbits -= 8
    if nbits:
        out.append(acc & 0xFF)
    return b"ESC2" + struct.pack("<6H", B, S, G, T, int(feat_shape[0]), int(feat_shape[1])) + bytes(counts) + bytes(out)


def ref_unpack_esc2(blob):
    B, S, G, T, H, W = struct.unpack("<6H", blob[4:16])
    counts = list(blob[16:16 + B])
    bits = int.from_bytes(blob[16 + B:], "little")
    codes = np.full((B, S, G, T), -1, np.int64)
    i = 0
    for b in range(B):
        n = counts[b] * G * T
        vals = [(bits >> (10 * (i + k))) & 1023 for k in range(n)]
        codes[b, :counts[b]] = np.array(vals, np.int64).reshape(counts[b], G, T)
        i += n
    return codes, (H, W), counts


def _random_padded(B, S, G, T, counts, seed):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 1024, (B, S, G, T)).astype(np.int64)
    for b, s in enumerate(counts):
        c[b, s:] = -1
    return c


# ------------------------------------------------------------------ CPU ---------------------------------------------------------
def test_esc2_header_and_sizes_against_reference_unpacker():
    from esc import bitstream
    for (B, S, G, T), counts in [((3, 6, 3, 150), [1, 6, 4]), ((5, 4, 3, 7), [4, 1, 1, 3, 2]), ((1, 1, 3, 1), [1]), ((2, 3, 2, 5), [3, 3])]:
        codes = _random_padded(B, S, G, T, counts, seed=B * 100 + S)
        blob = ref_pack_esc2(codes, (2, 2 * T), counts)
        n = sum(counts) * G * T
        payload = (10 * n + 7) // 8
        assert len(blob) == bitstream.HEADER_BYTES + B + payload
        hdr = bitstream.parse_header2(blob)
        assert hdr == (B, S, G, T, 2, 2 * T, counts, bitstream.HEADER_BYTES + B, payload)
        back, shape, cnt = ref_unpack_esc2(blob)
        assert np.array_equal(back, codes) and shape == (2, 2 * T) and cnt == counts
        with pytest.raises(ValueError):
            bitstream.parse_header2(blob[:-1])                                   # truncated payload
        with pytest.raises(ValueError):
            bitstream.parse_header2(blob[:16 + B - 1])                           # counts cut off
        bad = bytearray(blob); bad[16] = S + 1
        with pytest.raises(ValueError):
            bitstream.parse_header2(bytes(bad))                                  # a count above the header's S
        bad[16] = 0
        with pytest.raises(ValueError):
            bitstream.parse_header2(bytes(bad))                                  # a clip with no stream
        with pytest.raises(ValueError):
            bitstream.parse_header(blob)                                         # not an ESC1 stream
    # bits per second of a mixed batch: 10 bits per transmitted code
    assert 10 * (1 + 6) * 3 * 150 / 3.0 / 2 == (bitstream.payload_bits_per_second(1) + bitstream.payload_bits_per_second(6)) / 2


def _cpu_model():
    from esc.models import make_model
    g = load_golden("base")
    model = make_model(json.loads(str(g["config_json"])))
    model.load_state_dict(synth_state("base"))
    return model.eval()


def test_per_clip_argument_validation_without_device():
    model = _cpu_model()
    x = torch.zeros(3, 48000)
    for bad in ([1, 2], [1, 2, 3, 4], [0, 1, 2], [1, 7, 2], [1.0, 2.0, 3.0], [1, True, 2], torch.tensor([[1, 2, 3]]),
                torch.tensor([1.0, 2.0, 3.0]), torch.tensor([1, 2])):
        with pytest.raises(ValueError):
            model.encode(x, bad)
        with pytest.raises(ValueError):
            model(x, None, bad)
    with pytest.raises(ValueError):
        model.decode(torch.zeros(3, 4, 3, 150, dtype=torch.int64), (2, 300), num_streams=[1, 5, 2])     # more streams than code slots
    with pytest.raises(ValueError):
        model.decode(torch.zeros(3, 4, 3, 150, dtype=torch.int64), (2, 300), num_streams=[1, 2])
    with pytest.raises(ValueError):
        model.decode(torch.zeros(3, 4, 3, 150, dtype=torch.int64), (2, 300), num_streams=4)            # a uniform count is codes.size(1)
    # accepted forms get as far as the device check (no CPU implementation)
    for ok in ([1, 6, 3], (2, 2, 2), torch.tensor([1, 2, 3]), np.array([6, 1, 1], np.int32), range(1, 4)):
        with pytest.raises(RuntimeError, match="HIP device"):
            model.encode(x, ok)
    with pytest.raises(RuntimeError, match="HIP device"):
        model.encode(x, np.int64(3))                                           # a scalar is the uniform path
    # training mode: one num_streams per batch (scripts/utils.py:11-25)
    model.train()
    for seq in ([1, 2, 3], torch.tensor([3, 3, 3])):
        with pytest.raises(ValueError, match="per-clip"):
            model(x, None, seq)


def _gather_worker(rank, world, port, out_dir):
    sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
    import torch.distributed as dist
    from esc.distributed import all_gather_codes
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    counts = [[1, 6, 3], [6, 2, 4]]
    full = torch.from_numpy(np.concatenate([_random_padded(3, 6, 3, 150, counts[r], seed=10 + r) for r in range(world)]))
    local = full[3 * rank: 3 * rank + 3].contiguous()
    got = all_gather_codes(local)
    ragged = all_gather_codes(local[: 3 - rank].contiguous(), counts=[3, 2])
    ok = torch.equal(got, full) and torch.equal(ragged, torch.cat([full[:3], full[3:5]])) and int((got == -1).sum()) == int((full == -1).sum())
    np.save(os.path.join(out_dir, f"ok{rank}.npy"), np.array([int(ok)]))
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_all_gather_keeps_the_minus_one_fill(tmp_path):
    """Padded mixed-stream codes (-1 past each clip's count) cross the int16 all-gather of esc.distributed unchanged."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_gather_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    assert all(int(np.load(tmp_path / f"ok{r}.npy")[0]) == 1 for r in range(2))


# ------------------------------------------------------------------ GPU ---------------------------------------------------------
@pytest.fixture(scope="module")
def base():
    return build_models("base")


def _bench_clips(n, tag="mixed"):
    from esc import synth
    pcm = np.stack([synth.noise_clip_int16(f"{tag}-{i}", 48000, amp=0.04 + 0.01 * (i % 5)) for i in range(n)])
    return torch.from_numpy(synth.pcm_to_float(pcm)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", ["base", "large"])
def test_mixed_counts_against_golden(name, precision):
    """The reference's golden clips, each repeated at every count 1..6 in one batch: codes[b, :S_b] are the fixture's codes bit for bit,
    codes[b, S_b:] are -1, and the mixed decode matches the fixture audio of each clip's own count."""
    from esc import synth
    model, _, g, cfg = build_models(name, precision)
    S = cfg["max_streams"]
    n_clip = g["pcm"].shape[0]
    idx = [c for s in range(1, S + 1) for c in range(n_clip)]
    counts = [s for s in range(1, S + 1) for _ in range(n_clip)][::-1]          # mixed order: descending counts first, then reversed rows
    idx = idx[::-1]
    x = torch.from_numpy(synth.pcm_to_float(g["pcm"][idx])).cuda()
    codes, shape = model.encode(x, counts)
    assert codes.shape == (len(idx), S, 3, 150) and tuple(shape) == tuple(int(v) for v in g["feat_shape"])
    got = codes.cpu().numpy()
    for b, (c, s) in enumerate(zip(idx, counts)):
        ref = g["codes"][c, :s].astype(np.int64)
        assert np.array_equal(got[b, :s], ref), f"{name} clip {c} S={s}: " + code_report(got[b, :s], ref, g["margins"][c, :s])
        assert (got[b, s:] == -1).all()
    wave = model.decode(codes, shape, num_streams=counts).cpu().numpy()
    for b, (c, s) in enumerate(zip(idx, counts)):
        gold = g[f"audio_s{s}"][c]
        w = wave[b] if s == S else wave[b, ::8]
        assert rms(w, gold) <= AUDIO_TOL, f"{name} clip {c} S={s}: audio rms {rms(w, gold):.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_mixed_batch_rows_equal_uniform_calls(base, precision):
    """36 bench-sized clips with counts cycling 1..6: every row of the mixed encode / decode / forward (waveform and spectrum forms) is bit for bit
    the row of the uniform call at that clip's count on the same 36 clips."""
    model = base[0]
    model.set_precision(precision)
    x = _bench_clips(36)
    counts = [1 + (b * 5) % 6 for b in range(36)]
    mc, shape = model.encode(x, counts)
    md, mfeat = model.decode(mc, shape, return_feat=True, num_streams=counts)
    mf = model(x, None, counts)
    spec = mf["raw_feat"].permute(0, 2, 3, 1).contiguous()                   # (B, F, T, 2): the reference's x_feat layout
    mff = model(x, spec, counts)
    assert mc.shape == (36, 6, 3, 150) and mf["codes"].shape == (36, 6, 3, 150) and mff["codes"].shape == (36, 6, 3, 150)
    for s in range(1, 7):
        rows = [b for b in range(36) if counts[b] == s]
        uc, _ = model.encode(x, s)
        ud, ufeat = model.decode(uc, shape, return_feat=True)
        uf = model(x, None, s)
        uff = model(x, spec, s)
        for b in rows:
            assert torch.equal(mc[b, :s], uc[b]) and (mc[b, s:] == -1).all(), f"S={s} clip {b}: encode codes"
            assert torch.equal(md[b], ud[b]) and torch.equal(mfeat[b], ufeat[b]), f"S={s} clip {b}: decode"
            for o, u, form in ((mf, uf, "wave"), (mff, uff, "feat")):
                assert torch.equal(o["codes"][b, :s], u["codes"][b]) and (o["codes"][b, s:] == -1).all(), f"S={s} clip {b}: forward({form}) codes"
                for k in ("recon_audio", "recon_feat", "cm_loss", "cb_loss", "raw_feat"):
                    assert torch.equal(o[k][b], u[k][b]), f"S={s} clip {b}: forward({form}) {k}"


@pytest.mark.gpu
@pytest.mark.parametrize("precision", PRECISIONS)
def test_untransmitted_slots_are_not_read(base, precision):
    """Slots at or past S_b hold garbage (random codes, out-of-range values): the mixed decode gives the same audio and spectrum."""
    model = base[0]
    model.set_precision(precision)
    x = _bench_clips(12, "slots")
    counts = [1 + (b * 7) % 6 for b in range(12)]
    codes, shape = model.encode(x, counts)
    w0, f0 = model.decode(codes, shape, return_feat=True, num_streams=counts)
    g = torch.Generator(device="cpu").manual_seed(5)
    junk = torch.randint(-3000, 5000, codes.shape, generator=g).cuda()
    keep = torch.arange(6, device="cuda")[None, :, None, None] < torch.tensor(counts, device="cuda")[:, None, None, None]
    w1, f1 = model.decode(torch.where(keep, codes, junk), shape, return_feat=True, num_streams=counts)
    assert torch.equal(w0, w1) and torch.equal(f0, f1)
    # fewer code slots than 6 in the tensor (codes.size(1) = max count) works the same
    c4 = torch.where(keep, codes, junk)[:, :4].contiguous()
    c4_counts = [min(s, 4) for s in counts]
    w2 = model.decode(c4, shape, num_streams=c4_counts)
    ref4 = model.decode(codes[:, :4].clamp(min=0).contiguous(), shape, num_streams=c4_counts)
    assert torch.equal(w2, ref4)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [36, 288])
def test_uniform_list_equals_int(base, B):
    """A list of identical counts takes the mixed launch sequence (clip permutation, per-pass prefixes) and must match the int call bit for bit;
    288 clips run as two parts of several passes."""
    model = base[0]
    model.set_precision("f16x2")
    x = _bench_clips(B, "uniform")
    for s in (6, 3):
        c_int, shape = model.encode(x, s)
        c_lst, shape2 = model.encode(x, [s] * B)
        assert tuple(shape) == tuple(shape2) and torch.equal(c_int, c_lst)
        assert torch.equal(model.decode(c_int, shape), model.decode(c_lst, shape, num_streams=torch.full((B,), s)))
        if B == 36:
            a, b = model(x, None, s), model(x, None, [s] * B)
            for k in ("codes", "recon_audio", "recon_feat", "raw_feat", "cm_loss"):
                assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
def test_c_abi_errors_leave_the_handle_usable(base):
    from esc import _native, synth
    model, _, g, _ = base
    model.set_precision("f16x2")
    lib, hd = model._handle(torch.device("cuda:0"))
    x = torch.from_numpy(synth.pcm_to_float(g["pcm"])).cuda()
    codes = torch.zeros(2, 6, 3, 150, dtype=torch.int64, device="cuda")
    wave = torch.zeros(2, 47920, device="cuda")
    fh, fw = ctypes.c_int(), ctypes.c_int()
    E = _native.ESCX_ERR_INVALID_ARG
    for bad in ([0, 3], [3, 7], [-1, 1], None):
        cnt = _counts(bad) if bad is not None else None
        assert lib.escx_encode_streams(hd, _ptr(x), 2, 48000, cnt, _ptr(codes), ctypes.byref(fh), ctypes.byref(fw), _stream()) == E
        assert lib.escx_decode_streams(hd, _ptr(codes), 2, 6, cnt, 2, 300, _ptr(wave), None, _stream()) == E
        assert lib.escx_forward_streams(hd, _ptr(x), None, 2, 48000, cnt, _ptr(codes), _ptr(wave), None, None, None, _stream()) == E
    ok = _counts([6, 2])
    assert lib.escx_encode_streams(hd, None, 2, 48000, ok, _ptr(codes), None, None, _stream()) == E
    assert lib.escx_encode_streams(hd, _ptr(x), 0, 48000, ok, _ptr(codes), None, None, _stream()) == E
    assert lib.escx_decode_streams(hd, _ptr(codes), 2, 1, ok, 2, 300, _ptr(wave), None, _stream()) == E              # smax below a count
    assert lib.escx_decode_streams(hd, None, 2, 6, ok, 2, 300, _ptr(wave), None, _stream()) == E
    assert lib.escx_forward_streams(hd, _ptr(x), _ptr(x), 2, 48000, ok, _ptr(codes), _ptr(wave), None, None, None, _stream()) == E   # both inputs
    assert lib.escx_forward_streams(hd, None, None, 2, 48000, ok, _ptr(codes), _ptr(wave), None, None, None, _stream()) == E
    assert lib.escx_decode_streams(hd, _ptr(codes), 2, 6, ok, 2, 301, _ptr(wave), None, _stream()) == _native.ESCX_ERR_ASSERT   # overlap
    # the handle still gives the reference codes
    c, _ = model.encode(x, [6, 2])
    ref = g["codes"].astype(np.int64)
    assert np.array_equal(c[0].cpu().numpy(), ref[0]) and np.array_equal(c[1, :2].cpu().numpy(), ref[1, :2]) and (c[1, 2:] == -1).all().item()
    c6, _ = model.encode(x, 6)
    assert np.array_equal(c6.cpu().numpy(), ref)


@pytest.mark.gpu
def test_esc2_wire_round_trip(base):
    from esc import bitstream
    model = base[0]
    x = _bench_clips(7, "wire")
    counts = [3, 1, 6, 2, 6, 5, 4]
    codes, shape = model.encode(x, counts)
    blob = bitstream.pack_codes(codes, shape, num_streams=counts)
    n = sum(counts) * 3 * 150
    assert blob[:4] == b"ESC2" and len(blob) == bitstream.HEADER_BYTES + 7 + (10 * n + 7) // 8
    assert blob == ref_pack_esc2(codes.cpu().numpy(), shape, counts)
    back, shp, cnt = bitstream.unpack_codes(blob, model=model)
    assert torch.equal(back, codes) and tuple(shp) == tuple(shape) and cnt == counts
    assert torch.equal(model.decode(back, shp, num_streams=cnt), model.decode(codes, shape, num_streams=counts))
    # a code count that is not a multiple of 4 (the packer's last 5-byte group is cut to whole bytes)
    odd = torch.from_numpy(_random_padded(3, 2, 3, 3, [1, 2, 2], seed=3)).cuda()
    blob_odd = bitstream.pack_codes(odd, (2, 6), num_streams=[1, 2, 2])
    assert len(blob_odd) == 16 + 3 + (10 * 45 + 7) // 8 and blob_odd == ref_pack_esc2(odd.cpu().numpy(), (2, 6), [1, 2, 2])
    assert torch.equal(bitstream.unpack_codes(blob_odd)[0], odd)
    # ESC1 is unchanged
    full, _ = model.encode(x, 6)
    b1 = bitstream.pack_codes(full, shape)
    assert b1[:4] == b"ESC1" and len(b1) == 16 + 5 * ((7 * 6 * 3 * 150 + 3) // 4)
    with pytest.raises(ValueError):
        bitstream.pack_codes(codes, shape, num_streams=[7, 1, 1, 1, 1, 1, 1])
