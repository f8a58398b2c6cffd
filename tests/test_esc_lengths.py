"""Mixed-length batches of esc.ESC on the MI355X (`lengths` in encode / eval forward, `frame_lengths` in decode; include/escx.h escx_encode_lengths,
escx_decode_lengths, escx_forward_lengths).

The contract: (1) a clip gets its own answer - the codes of the oracle run on that clip alone (on these inputs no oracle argmin margin is below 1e-5,
asserted below, so no code may differ) and audio within the project's 1e-4 RMS of it; (2) a clip's result is a function of its own samples, its
length, Wmax, num_streams and the precision mode and of nothing else, bit for bit: not of the batch size, the order, the other clips, what x holds
past its length, or what the code tensor holds past its frames; (3) in every precision mode.

Lengths (W on the CPU oracle): tiny [1280, 70, 490, 570, 1279] -> 32, 2, 12, 14, 32 (a multiple of 4, one window column, a padded last window, a
dropped odd frame); ESC-Base [8000, 7680, 4080, 560, 2240] -> 50, 48, 26, 4, 14 (H = 2 at the bottom scale)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from gpu_util import PRECISIONS, build_models, have_gpu, rel_rms, rms

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not have_gpu(), reason="needs the MI355X")]

LENGTHS = {"tiny": [1280, 70, 490, 570, 1279], "base": [8000, 7680, 4080, 560, 2240]}
WIDTHS = {"tiny": [32, 2, 12, 14, 32], "base": [50, 48, 26, 4, 14]}
AUDIO_TOL = 1e-4          # the project's bound on decoded audio against the oracle (tests/test_gpu_parity.py)
LOSS_RTOL = 1e-4          # tests/test_gpu_parity.py test_forward_eval_dict compares cm_loss to the oracle's at this rtol
ACT_TOL, FEAT_TOL = 2e-5, 1e-4      # relative RMS of raw_feat / recon_feat against the oracle, as test_forward_eval_dict bounds them
CASES = [(n, p) for n in ("tiny", "base") for p in PRECISIONS]


def _clip(L):
    from esc import synth
    return torch.from_numpy(synth.pcm_to_float(synth.voiced_clip_int16(f"len{L}", L))).reshape(-1)


@functools.lru_cache(maxsize=None)
def _ctx(name):
    """model, per-clip oracle results (computed once per configuration and never modified), the batch."""
    from oracle.esc_oracle import Trace
    model, orc, g, cfg = build_models(name)
    S = cfg["max_streams"]
    clips = [_clip(L) for L in LENGTHS[name]]
    ref = []
    for c in clips:
        tr = Trace()
        codes, shape = orc.encode(c[None], S, trace=tr)
        out = orc.forward_eval(c[None], None, S)
        assert torch.equal(out["codes"], codes)
        ref.append({"codes": codes[0].numpy(), "shape": tuple(shape), "margin": float(torch.stack(tr.margins, dim=1).min()),
                    "audio": out["recon_audio"][0].numpy(), "cm": float(out["cm_loss"][0]), "cb": float(out["cb_loss"][0]),
                    "raw_feat": out["raw_feat"][0].numpy(), "recon_feat": out["recon_feat"][0].numpy()})
    return {"model": model, "orc": orc, "cfg": cfg, "S": S, "clips": clips, "ref": ref}


def _batch(clips, fill=0.0, Lx=None):
    Lx = Lx or max(len(c) for c in clips)
    x = torch.full((len(clips), Lx), fill, dtype=torch.float32)
    for b, c in enumerate(clips):
        x[b, :len(c)] = c
    return x.cuda()


def _setup(name, precision):
    c = _ctx(name)
    c["model"].set_precision(precision)
    return c, c["model"], LENGTHS[name], WIDTHS[name]


def _forward(model, x, S, lengths):
    return model(**dict(x=x, x_feat=None, num_streams=S, lengths=lengths))


OUT_KEYS = ("codes", "recon_audio", "cm_loss", "cb_loss", "raw_feat", "recon_feat")


@pytest.mark.parametrize("name,precision", CASES)
def test_encode_codes_are_the_clips_own(name, precision):
    c, model, L, W = _setup(name, precision)
    ov = c["cfg"]["overlap"]
    codes, shape = model.encode(_batch(c["clips"]), c["S"], lengths=L)
    assert tuple(shape) == (c["ref"][0]["shape"][0], max(W)) and codes.shape == (len(L), c["S"], c["cfg"]["group_size"], max(W) // ov)
    assert model.frame_lengths(L) == W and [r["shape"][1] for r in c["ref"]] == W
    got = codes.cpu().numpy()
    print(f"{name}: smallest oracle argmin margin {min(r['margin'] for r in c['ref']):.3e}")
    for b, r in enumerate(c["ref"]):
        assert r["margin"] > 1e-5, "precondition: no oracle argmin on these clips is a near-tie, so no code may differ"
        own = got[b, :, :, :W[b] // ov]
        assert np.array_equal(own, r["codes"]), f"clip {b} (L={L[b]}): {int((own != r['codes']).sum())} of {own.size} codes differ from the oracle on the clip alone"
        assert (got[b, :, :, W[b] // ov:] == -1).all(), f"clip {b}: codes past its frames are not -1"


@pytest.mark.parametrize("name,precision", CASES)
def test_decode_audio_is_the_clips_own_and_zero_past_it(name, precision):
    c, model, L, W = _setup(name, precision)
    codes, shape = model.encode(_batch(c["clips"]), c["S"], lengths=L)
    wave, feat = model.decode(codes, shape, return_feat=True, frame_lengths=W)
    n_out = model.output_lengths(W)
    pt = c["cfg"]["patch_size"][1]
    assert wave.shape == (len(L), max(n_out)) and feat.shape[-1] == pt * max(W)
    wave, feat = wave.cpu().numpy(), feat.cpu().numpy()
    for b, r in enumerate(c["ref"]):
        assert n_out[b] == len(r["audio"])
        e = rms(wave[b, :n_out[b]], r["audio"])
        print(f"{name} {precision} clip {b}: decode audio rms {e:.3e}")
        assert e <= AUDIO_TOL, (b, e)
        assert (wave[b, n_out[b]:] == 0).all(), f"clip {b}: audio past its own output is not exactly 0"
        assert rel_rms(feat[b, :, :, :pt * W[b]], r["recon_feat"]) < FEAT_TOL
        assert (feat[b, :, :, pt * W[b]:] == 0).all()


@pytest.mark.parametrize("name,precision", CASES)
def test_forward_is_the_composition_with_per_clip_losses(name, precision):
    c, model, L, W = _setup(name, precision)
    x = _batch(c["clips"])
    out = _forward(model, x, c["S"], L)
    assert set(out) == {"cm_loss", "cb_loss", "raw_audio", "recon_audio", "raw_feat", "recon_feat", "codes"}
    codes, shape = model.encode(x, c["S"], lengths=L)
    assert torch.equal(out["codes"], codes)
    assert torch.equal(out["recon_audio"], model.decode(codes, shape, frame_lengths=W)), "forward must equal decode(encode()) bit for bit"
    hop, pt = model.hop_length, c["cfg"]["patch_size"][1]
    n_out = model.output_lengths(W)
    wave, cm, cb = out["recon_audio"].cpu().numpy(), out["cm_loss"].cpu().numpy(), out["cb_loss"].cpu().numpy()
    raw, rec = out["raw_feat"].cpu().numpy(), out["recon_feat"].cpu().numpy()
    assert raw.shape[-1] == 1 + max(L) // hop and rec.shape[-1] == pt * max(W)
    for b, r in enumerate(c["ref"]):
        e = rms(wave[b, :n_out[b]], r["audio"])
        print(f"{name} {precision} clip {b}: forward audio rms {e:.3e}, cm_loss {cm[b]:.6e} (oracle {r['cm']:.6e})")
        assert e <= AUDIO_TOL and (wave[b, n_out[b]:] == 0).all()
        np.testing.assert_allclose(cm[b], r["cm"], rtol=LOSS_RTOL)
        np.testing.assert_allclose(cb[b], r["cb"], rtol=LOSS_RTOL)
        Tb = 1 + L[b] // hop
        assert rel_rms(raw[b, :, :, :Tb], r["raw_feat"]) < ACT_TOL and rel_rms(rec[b, :, :, :pt * W[b]], r["recon_feat"]) < FEAT_TOL
        assert (raw[b, :, :, Tb:] == 0).all() and (rec[b, :, :, pt * W[b]:] == 0).all()


@pytest.mark.parametrize("name,precision", CASES)
def test_a_clips_result_does_not_depend_on_the_batch(name, precision):
    """Bitwise: a permuted batch, the two-clip batch [clip 0, clip 3] (same Wmax), x filled with NaN past each length, and the same call twice."""
    c, model, L, W = _setup(name, precision)
    S, clips = c["S"], c["clips"]
    ref = _forward(model, _batch(clips), S, L)
    again = _forward(model, _batch(clips), S, L)
    nan = _forward(model, _batch(clips, fill=float("nan")), S, L)
    for k in OUT_KEYS:
        assert torch.equal(ref[k], again[k]), f"{k}: two identical calls differ"
        assert torch.equal(ref[k], nan[k]), f"{k} depends on what x holds past a clip's length"
        assert not torch.isnan(ref[k].float()).any()
    perm = [3, 0, 4, 2, 1]
    p = _forward(model, _batch([clips[i] for i in perm]), S, [L[i] for i in perm])
    for k in OUT_KEYS:
        assert torch.equal(p[k], ref[k][perm]), f"{k} depends on the order of the clips"
    two = _forward(model, _batch([clips[0], clips[3]]), S, [L[0], L[3]])
    for k in OUT_KEYS:
        assert torch.equal(two[k], ref[k][[0, 3]]), f"{k} depends on the batch size / the other clips"
    codes, shape = model.encode(_batch(clips, fill=float("nan")), S, lengths=L)
    assert torch.equal(codes, ref["codes"])


@pytest.mark.parametrize("name,precision", CASES)
def test_decode_never_reads_the_dead_code_slots(name, precision):
    c, model, L, W = _setup(name, precision)
    ov = c["cfg"]["overlap"]
    codes, shape = model.encode(_batch(c["clips"]), c["S"], lengths=L)
    ref = model.decode(codes, shape, return_feat=True, frame_lengths=W)
    other = codes.clone()
    fillv = torch.arange(other.numel(), device=other.device).reshape(other.shape) % c["cfg"]["codebook_size"]     # valid indices only
    for b in range(len(L)):
        other[b, :, :, W[b] // ov:] = fillv[b, :, :, W[b] // ov:]
    assert (other >= 0).all() and (other < c["cfg"]["codebook_size"]).all()
    got = model.decode(other, shape, return_feat=True, frame_lengths=W)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
    assert torch.equal(model.decode(codes, shape, frame_lengths=torch.tensor(W)), ref[0])


@pytest.mark.parametrize("name,precision", CASES)
def test_equal_lengths_give_the_plain_calls_codes(name, precision):
    c, model, L, W = _setup(name, precision)
    S = c["S"]
    x = _batch([c["clips"][0], c["clips"][0].flip(0)])
    Lx = x.shape[1]
    plain, pshape = model.encode(x, S)
    codes, shape = model.encode(x, S, lengths=[Lx, Lx])
    assert tuple(shape) == tuple(pshape) and torch.equal(codes, plain)
    wave = model.decode(codes, shape, frame_lengths=[shape[1]] * 2).cpu()
    ow = c["orc"].decode(codes.cpu(), shape)
    e = rms(wave.numpy(), ow.numpy())
    print(f"{name} {precision}: equal lengths audio rms {e:.3e}")
    assert e <= AUDIO_TOL


@pytest.mark.parametrize("name", ("tiny", "base"))
def test_c_entry_points_refuse_bad_arguments_and_leave_the_handle_usable(name):
    from esc import _native
    c, model, L, W = _setup(name, PRECISIONS[0])
    S, ov = c["S"], c["cfg"]["overlap"]
    x = _batch(c["clips"])
    B, Lx = x.shape
    before = model.encode(x, S)[0].clone()
    lib, hd = model._handle(x.device)
    st = model._stream(x.device)
    codes = torch.empty((B, S, c["cfg"]["group_size"], max(W) // ov), dtype=torch.int64, device=x.device)
    wave = torch.empty((B, model.output_lengths([max(W)])[0]), dtype=torch.float32, device=x.device)
    fh, fw = ctypes.c_int(), ctypes.c_int()
    arr = lambda v: (ctypes.c_int32 * len(v))(*v)
    odd = model.hop_length * (c["cfg"]["patch_size"][1] * 3)          # 3 latent frames: no multiple of overlap = 2
    H = c["ref"][0]["shape"][0]
    enc = lambda lens, b=B, s=S: lib.escx_encode_lengths(hd, x.data_ptr(), b, Lx, lens, s, codes.data_ptr(), ctypes.byref(fh), ctypes.byref(fw), st)
    dec = lambda ws, b=B: lib.escx_decode_lengths(hd, codes.data_ptr(), b, S, ws, H, max(W), wave.data_ptr(), None, st)
    fwd = lambda lens, b=B: lib.escx_forward_lengths(hd, x.data_ptr(), b, Lx, lens, S, codes.data_ptr(), wave.data_ptr(), None, None, None, st)
    with torch.cuda.device(x.device):
        assert enc(None) == _native.ESCX_ERR_INVALID_ARG and fwd(None) == _native.ESCX_ERR_INVALID_ARG and dec(None) == _native.ESCX_ERR_INVALID_ARG
        assert enc(arr(L), b=0) == _native.ESCX_ERR_INVALID_ARG
        assert enc(arr(L), s=0) == _native.ESCX_ERR_INVALID_ARG
        for bad in ([Lx + 1] + L[1:], L[:-1] + [model.in_freq - 1], L[:-1] + [-5]):
            assert enc(arr(bad)) == _native.ESCX_ERR_INVALID_ARG and fwd(arr(bad)) == _native.ESCX_ERR_INVALID_ARG
        assert enc(arr(L[:2] + [odd] + L[3:])) == _native.ESCX_ERR_ASSERT and b"clip 2" in lib.escx_last_error()
        assert fwd(arr(L[:2] + [odd] + L[3:])) == _native.ESCX_ERR_ASSERT
        assert dec(arr(W[:-1] + [max(W) + ov])) == _native.ESCX_ERR_INVALID_ARG and dec(arr([0] + W[1:])) == _native.ESCX_ERR_INVALID_ARG
        assert dec(arr(W[:-1] + [3])) == _native.ESCX_ERR_ASSERT
    assert torch.equal(model.encode(x, S)[0], before), "a refused call changed what the handle computes"
    with pytest.raises(AssertionError, match="clip 2"):
        model.encode(x, S, lengths=L[:2] + [odd] + L[3:])


@pytest.mark.parametrize("name", ("tiny", "base"))
def test_a_short_batch_after_a_long_one_sees_no_stale_workspace(name):
    c, model, L, W = _setup(name, PRECISIONS[0])
    S, ov = c["S"], c["cfg"]["overlap"]
    _forward(model, _batch(c["clips"]), S, L)                 # fills the workspace with the long batch
    idx = [1, 2]
    out = _forward(model, _batch([c["clips"][i] for i in idx]), S, [L[i] for i in idx])
    n_out = model.output_lengths([W[i] for i in idx])
    got, wave = out["codes"].cpu().numpy(), out["recon_audio"].cpu().numpy()
    for j, i in enumerate(idx):
        r = c["ref"][i]
        assert np.array_equal(got[j, :, :, :W[i] // ov], r["codes"]) and (got[j, :, :, W[i] // ov:] == -1).all()
        assert rms(wave[j, :n_out[j]], r["audio"]) <= AUDIO_TOL and (wave[j, n_out[j]:] == 0).all()
        np.testing.assert_allclose(out["cm_loss"][j].item(), r["cm"], rtol=LOSS_RTOL)


@pytest.mark.parametrize("name", ("tiny", "base"))
def test_the_unfused_attention_sequence_has_the_length_form(name, monkeypatch):
    """A width without a fused attention mode runs ln_rows / window_attention / gemm_proj_scatter on the same tables (the flags go to the attention core).
    ESCX_NO_FUSED_ATTN=1 (read when the handle is created) puts every layer on that sequence: same codes, same audio bound, same independence."""
    monkeypatch.setenv("ESCX_NO_FUSED_ATTN", "1")
    c = _ctx(name)
    model = build_models(name)[0]               # a fresh handle, created under the switch
    L, W, S, ov = LENGTHS[name], WIDTHS[name], c["S"], c["cfg"]["overlap"]
    out = _forward(model, _batch(c["clips"], fill=float("nan")), S, L)
    n_out = model.output_lengths(W)
    got, wave = out["codes"].cpu().numpy(), out["recon_audio"].cpu().numpy()
    for b, r in enumerate(c["ref"]):
        assert np.array_equal(got[b, :, :, :W[b] // ov], r["codes"]) and (got[b, :, :, W[b] // ov:] == -1).all()
        e = rms(wave[b, :n_out[b]], r["audio"])
        print(f"{name} unfused attention clip {b}: audio rms {e:.3e}")
        assert e <= AUDIO_TOL and (wave[b, n_out[b]:] == 0).all()
        np.testing.assert_allclose(out["cm_loss"][b].item(), r["cm"], rtol=LOSS_RTOL)
    two = _forward(model, _batch([c["clips"][0], c["clips"][3]]), S, [L[0], L[3]])
    for k in OUT_KEYS:
        assert torch.equal(two[k], out[k][[0, 3]]), f"{k} depends on the batch (unfused attention)"
