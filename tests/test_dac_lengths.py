"""Mixed-length batches of the DAC baseline (esc.baselines.DAC) on the MI355X, in fp32 and bf16x3: with per-clip lengths every clip of encode,
quantizer.from_codes, decode and forward is bitwise the uniform call on that clip alone (include/escx.h escx_dac_encode_lengths,
escx_dac_from_codes_lengths, escx_dac_decode_lengths).  Also: the fillers past a clip's length, the losses as the mean of the single-clip calls',
NaN and junk past a clip's length (never read), determinism, permutation, equal lengths against the plain call, the very short clips against the
torch restatement under the near-tie rule, and the argument errors of the three C entry points."""
import ctypes
import json

import numpy as np
import pytest
import torch

import dac_util as du
from conftest import load_golden, load_manifest
from esc import synth

pytestmark = pytest.mark.gpu
PRECISIONS = ("fp32", "bf16x3")
_MODELS = {}
# dac_syn (hop 4): frames 400, 9, 94, 1, 200, 401 of Tmax = 401; the geometry is asserted in test_geometry_of_the_syn_batch
SYN_LENGTHS = [1603, 37, 377, 4, 801, 1604]
TINY_LENGTHS = [4800, 321, 3200, 960]                      # dac_tiny (hop 320): frames 15, 1, 10, 3
TINY_COUNTS = [18, 1, 6, 12]


def _cfg(name):
    return json.loads(str(load_golden(name)["config_json"]))


def _sd(name):
    return {k: torch.from_numpy(v) for k, v in synth.dac_state_dict(load_manifest(name)).items()}


def _new_model(name):
    from esc.baselines import DAC
    m = DAC(**_cfg(name))
    m.load_state_dict(_sd(name), strict=True)
    return m.cuda().eval()


@pytest.fixture
def model(request):
    """(name, precision) -> the shared model of that configuration in that precision; fp32 is restored afterwards."""
    used = []

    def get(name, precision):
        if name not in _MODELS:
            _MODELS[name] = _new_model(name)
        used.append(_MODELS[name])
        return _MODELS[name].set_precision(precision)
    yield get
    for m in used:
        m.set_precision("fp32")


def _batch(name, lengths):
    """(B, 1, max(lengths)) audio: one synthesised clip per row (noise / voiced in turn), zeros past its length."""
    x = np.zeros((len(lengths), max(lengths)), np.float32)
    for i, n in enumerate(lengths):
        pcm = (synth.voiced_clip_int16 if i % 2 else synth.noise_clip_int16)(f"dac-lengths-{name}-{i}", max(n, 64))
        x[i, :n] = synth.pcm_to_float(pcm[None])[0, :n]
    return torch.from_numpy(x)[:, None].cuda()


def _check_encode(m, x, lengths, counts=None):
    """Every clip of encode(x, counts, lengths) against the uniform call on that clip alone, the fillers and the losses; returns the batch's tuple."""
    d, B = m.codebook_dim, x.shape[0]
    z, codes, lat, cm, cb = out = m.encode(x, counts, lengths=lengths)
    ns = [m.n_codebooks] * B if counts is None else [min(int(n), m.n_codebooks) for n in counts]
    nmax, T = max(ns), m.num_frames(max(lengths))
    fl = m.frame_lengths(lengths).tolist()
    assert T == max(fl)
    assert z.shape == (B, m.latent_dim, T) and codes.shape == (B, nmax, T) and lat.shape == (B, nmax * d, T)
    assert codes.dtype == torch.int64 and cm.dim() == 0 and cb.dim() == 0
    solo_cm, solo_cb = [], []
    for b, (L, Tb, n) in enumerate(zip(lengths, fl, ns)):
        z1, c1, l1, cm1, cb1 = m.encode(x[b:b + 1, :, :L], n)
        assert z1.shape[-1] == Tb
        assert torch.equal(z[b:b + 1, :, :Tb], z1), b
        assert torch.equal(codes[b:b + 1, :n, :Tb], c1), b
        assert torch.equal(lat[b:b + 1, :n * d, :Tb], l1), b
        assert bool((z[b, :, Tb:] == 0).all()) and bool((lat[b, :, Tb:] == 0).all()) and bool((codes[b, :, Tb:] == -1).all()), b
        assert bool((codes[b, n:] == -1).all()) and bool((lat[b, n * d:] == 0).all()), b
        solo_cm.append(float(cm1)); solo_cb.append(float(cb1))
    print(f"losses {float(cm):.8g} {float(cb):.8g}  mean of the solo calls {np.mean(solo_cm):.8g} {np.mean(solo_cb):.8g}")
    np.testing.assert_allclose(float(cm), np.mean(solo_cm), rtol=1e-5)     # summation order over the clips, as in the per-clip-counts test
    np.testing.assert_allclose(float(cb), np.mean(solo_cb), rtol=1e-5)
    return out


def _check_round_trip(m, x, lengths, counts=None):
    """encode -> from_codes -> decode of the batch, every clip against the uniform calls on that clip alone."""
    d = m.codebook_dim
    z, codes, lat, _, _ = m.encode(x, counts, lengths=lengths)
    fl = m.frame_lengths(lengths)
    ol = m.output_lengths(fl).tolist()
    zq, zp, c = m.quantizer.from_codes(codes, counts, frame_lengths=fl)    # -1 past every clip's frames (and counts): neither read nor range-checked
    assert c is codes and zq.shape == z.shape and zp.shape == lat.shape
    audio = m.decode(zq, frame_lengths=fl)
    assert audio.shape == (x.shape[0], 1, m.output_samples(int(fl.max()))) and audio.shape[-1] == max(ol)
    for b, Tb in enumerate(fl.tolist()):
        n = codes.shape[1] if counts is None else min(int(counts[b]), m.n_codebooks)
        zq1, zp1, _ = m.quantizer.from_codes(codes[b:b + 1, :n, :Tb].contiguous())
        assert torch.equal(zq[b:b + 1, :, :Tb], zq1) and torch.equal(zp[b:b + 1, :n * d, :Tb], zp1), b
        assert bool((zq[b, :, Tb:] == 0).all()) and bool((zp[b, :, Tb:] == 0).all()) and bool((zp[b, n * d:] == 0).all()), b
        a1 = m.decode(zq[b:b + 1, :, :Tb].contiguous())
        assert a1.shape[-1] == ol[b]
        assert torch.equal(audio[b:b + 1, :, :ol[b]], a1), b
        assert bool((audio[b, :, ol[b]:] == 0).all()), b
    return zq, audio


def _check_forward(m, x, lengths, counts=None):
    out = m(x, None, counts, lengths=lengths)
    assert set(out) == {"audio", "z", "codes", "latents", "vq/commitment_loss", "vq/codebook_loss", "frame_lengths"}
    hop = m.hop_length
    fl = [m.num_frames(-(-L // hop) * hop) for L in lengths]                # every clip through preprocess on its own
    assert out["frame_lengths"].dtype == torch.int64 and out["frame_lengths"].device.type == "cpu" and out["frame_lengths"].tolist() == fl
    width = min(x.shape[-1], m.output_samples(max(fl)))
    assert out["audio"].shape == (x.shape[0], 1, width) and out["z"].shape[-1] == max(fl)
    for b, (L, Tb) in enumerate(zip(lengths, fl)):
        n = None if counts is None else int(counts[b])
        solo = m(x[b:b + 1, :, :L], None, n)
        k = solo["audio"].shape[-1]
        assert k == min(L, m.output_samples(Tb))
        assert torch.equal(out["audio"][b:b + 1, :, :k], solo["audio"]), b
        assert bool((out["audio"][b, :, k:] == 0).all()), b
        assert torch.equal(out["z"][b:b + 1, :, :Tb], solo["z"]), b
        nn = solo["codes"].shape[1]
        assert torch.equal(out["codes"][b:b + 1, :nn, :Tb], solo["codes"]), b
        assert torch.equal(out["latents"][b:b + 1, :nn * m.codebook_dim, :Tb], solo["latents"]), b
        assert bool((out["codes"][b, :, Tb:] == -1).all()) and bool((out["z"][b, :, Tb:] == 0).all()), b
    return out


def test_geometry_of_the_syn_batch():
    """What the dac_syn batch is meant to hit, on the latent-level row grid m = b * Tmax + t that the GEMM tiles and the quantiser workgroups cut."""
    from esc.baselines import DAC
    m = DAC(**_cfg("dac_syn"))
    assert m.hop_length == 4 and m.latent_dim == 32 and m.n_codebooks == 4
    fl = m.frame_lengths(SYN_LENGTHS).tolist()
    T = max(fl)
    assert fl == [400, 9, 94, 1, 200, 401] and T == 401
    ends = [b * T + t for b, t in enumerate(fl)]                            # the first dead row of every clip
    assert 1 in fl                                                          # a clip of a single frame
    assert any(e % 64 and e % 128 and e % 4 for e in ends)                  # an end inside a 64- / 128-row GEMM tile and a 4-row quantiser workgroup
    assert any(e % 128 == 0 for e in ends)                                  # an end on a tile edge (of both tile heights)
    dead = np.ones(len(fl) * T, bool)
    for b, t in enumerate(fl):
        dead[b * T:b * T + t] = False
    for bm in (64, 128):
        tiles = [dead[i:i + bm].all() for i in range(0, len(dead), bm)]
        assert any(tiles) and not all(tiles), bm                            # at least one tile without a live row
    assert len(dead) > 128                                                  # more than one workgroup


@pytest.mark.parametrize("precision", PRECISIONS)
def test_syn_every_clip_is_its_solo_call(model, precision):
    m = model("dac_syn", precision)
    x = _batch("dac_syn", SYN_LENGTHS)
    _check_encode(m, x, SYN_LENGTHS)
    _check_encode(m, x, torch.tensor(SYN_LENGTHS), [1, 4, 2, 4, 3, 1])
    _check_round_trip(m, x, SYN_LENGTHS)
    _check_forward(m, x, SYN_LENGTHS)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("counts", (None, TINY_COUNTS))
def test_tiny_every_clip_is_its_solo_call(model, precision, counts):
    """latent 512 (J = 8), 18 codebooks, hop 320; once with per-clip n_quantizers on top."""
    m = model("dac_tiny", precision)
    x = _batch("dac_tiny", TINY_LENGTHS)
    _check_encode(m, x, TINY_LENGTHS, counts)
    _check_round_trip(m, x, TINY_LENGTHS, counts)
    _check_forward(m, x, TINY_LENGTHS, counts)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,lengths", [("dac_syn", SYN_LENGTHS), ("dac_tiny", TINY_LENGTHS)])
def test_nothing_past_a_length_is_read(model, precision, name, lengths):
    m = model(name, precision)
    x = _batch(name, lengths)
    fl = m.frame_lengths(lengths).tolist()
    enc = m.encode(x, lengths=lengths)
    fwd = m(x, lengths=lengths)
    xp = x.clone()
    for b, L in enumerate(lengths):
        xp[b, :, L:] = float("nan")
    for a, b_ in zip(m.encode(xp, lengths=lengths), enc):
        assert torch.equal(a, b_) and bool(torch.isfinite(a.float()).all())
    fwd2 = m(xp, lengths=lengths)
    for k in ("audio", "z", "codes", "latents", "vq/commitment_loss", "vq/codebook_loss"):
        assert torch.equal(fwd2[k], fwd[k]) and bool(torch.isfinite(fwd2[k].float()).all()), k
    z, codes = enc[0], enc[1]
    audio = m.decode(z, frame_lengths=fl)
    zq, zp, _ = m.quantizer.from_codes(codes, frame_lengths=fl)
    zpn = z.clone()
    for b, t in enumerate(fl):
        zpn[b, :, t:] = float("nan")
    a2 = m.decode(zpn, frame_lengths=fl)
    assert torch.equal(a2, audio) and bool(torch.isfinite(a2).all())
    for junk in (-1, m.codebook_size + 1000, 2 ** 40):
        cj = codes.clone()
        for b, t in enumerate(fl):
            cj[b, :, t:] = junk
        zq2, zp2, _ = m.quantizer.from_codes(cj, frame_lengths=fl)
        assert torch.equal(zq2, zq) and torch.equal(zp2, zp) and bool(torch.isfinite(zq2).all()) and bool(torch.isfinite(zp2).all()), junk
    live = codes.clone(); live[0, 0, 0] = -1
    with pytest.raises(IndexError):
        m.quantizer.from_codes(live, frame_lengths=fl)                      # a slot that is read is still checked
    with pytest.raises(IndexError):
        m.quantizer.from_codes(codes)                                       # and without the lengths the -1 fillers still raise


@pytest.mark.parametrize("precision", PRECISIONS)
def test_determinism_permutation_and_equal_lengths(model, precision):
    m = model("dac_syn", precision)
    x = _batch("dac_syn", SYN_LENGTHS)
    a = m(x, lengths=SYN_LENGTHS)
    b = m(x, lengths=SYN_LENGTHS)
    keys = ("audio", "z", "codes", "latents", "vq/commitment_loss", "vq/codebook_loss")
    for k in keys:
        assert torch.equal(a[k], b[k]), k
    perm = [3, 5, 0, 2, 4, 1]
    p = m(x[perm].contiguous(), lengths=[SYN_LENGTHS[i] for i in perm])
    for k in keys[:4]:
        assert torch.equal(p[k], a[k][perm]), k
    assert p["frame_lengths"].tolist() == a["frame_lengths"][perm].tolist()
    np.testing.assert_allclose(float(p[keys[4]]), float(a[keys[4]]), rtol=1e-5)      # the clips' means are added in another order
    # all lengths equal to L: the plain call
    for L in (1603, 1604):
        xe = x[:3, :, :L].contiguous()
        for got, want in zip(m.encode(xe, lengths=[L] * 3), m.encode(xe)):
            assert torch.equal(got, want), L
        for got, want in zip(m.encode(xe, [1, 4, 2], lengths=[L] * 3), m.encode(xe, [1, 4, 2])):
            assert torch.equal(got, want), L
        fo, fp = m(xe, lengths=[L] * 3), m(xe)
        for k in keys:
            assert torch.equal(fo[k], fp[k]), (L, k)
        z = fp["z"]
        T = z.shape[-1]
        assert torch.equal(m.decode(z, frame_lengths=[T] * 3), m.decode(z))
        for got, want in zip(m.quantizer.from_codes(fp["codes"], frame_lengths=[T] * 3)[:2], m.quantizer.from_codes(fp["codes"])[:2]):
            assert torch.equal(got, want)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_short_clips_against_the_restatement(model, precision):
    """The dac_syn clips - down to one frame, which no fixture covers - against tests/dac_util.DacRef run on each sliced clip, under the project's
    near-tie rule (tol 2e-6): no violation."""
    m = model("dac_syn", precision)
    x = _batch("dac_syn", SYN_LENGTHS)
    codes = m.encode(x, lengths=SYN_LENGTHS)[1].cpu().numpy()
    ref = du.DacRef(_cfg("dac_syn"), _sd("dac_syn"))
    n, attributed = m.n_codebooks, 0
    for b, L in enumerate(SYN_LENGTHS):
        with torch.no_grad():
            z_enc = ref.encoder(x[b:b + 1, :, :L].cpu())
            want = ref.quantize(z_enc, n, margins=True)
        Tb = z_enc.shape[-1]
        assert Tb == m.num_frames(L)
        rows, bad = du.attribute_codes(ref, z_enc, n, codes[b:b + 1, :, :Tb], want[1].numpy(), want[5].numpy())
        assert not bad, f"clip {b} ({L} samples): codes differ beyond the near-tie rule: {bad[:5]}"
        attributed += rows
    print(f"{precision}: {attributed} attributed rows over {len(SYN_LENGTHS)} clips")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_c_abi_argument_errors_leave_the_handle_usable(model, precision):
    from esc import _native
    lib = _native.load()
    m = _new_model("dac_syn").set_precision(precision)
    lengths = SYN_LENGTHS[:3]
    x = _batch("dac_syn", lengths).contiguous()
    B, L, nc, d = 3, x.shape[-1], m.n_codebooks, m.codebook_dim
    T = m.num_frames(L)
    _, hd, flat, dev, stream = m._ctx(x, "x")
    z = torch.zeros(B, m.latent_dim, T, device="cuda")
    codes = torch.zeros(B, nc, T, dtype=torch.int64, device="cuda")
    lat = torch.empty(B, nc * d, T, device="cuda")
    losses = torch.empty(2, device="cuda")
    audio = torch.empty(B, m.output_samples(T), device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    arr = lambda v: None if v is None else (ctypes.c_int32 * len(v))(*v)         # noqa: E731

    def enc(lens, batch=B, clip_n=None, pad=1):
        return lib.escx_dac_encode_lengths(hd, p(flat), m._version(), p(x), batch, L, arr(lens), pad, nc, arr(clip_n), p(z), p(codes), p(lat), p(losses), stream)

    def frc(fl, batch=B, clip_n=None):
        return lib.escx_dac_from_codes_lengths(hd, p(flat), m._version(), p(codes), batch, nc, T, arr(fl), arr(clip_n), p(z), p(lat), stream)

    def dec(fl, batch=B, caps=None):
        return lib.escx_dac_decode_lengths(hd, p(flat), m._version(), p(z), batch, T, arr(fl), arr(caps), p(audio), stream)

    bad = _native.ESCX_ERR_INVALID_ARG
    assert enc(None) == bad and frc(None) == bad and dec(None) == bad                   # a null array
    assert enc(lengths, batch=0) == bad and frc([T] * 3, batch=0) == bad and dec([T] * 3, batch=0) == bad
    assert enc([L, 0, 4]) == bad and b"lengths[1]" in lib.escx_last_error()             # outside [1, Lmax]
    assert enc([L, 4, L + 1]) == bad and b"lengths[2]" in lib.escx_last_error()
    assert enc([3, L, L]) == bad and b"lengths[0]" in lib.escx_last_error()             # below one hop: no frame
    assert enc(lengths, pad=0) == bad
    assert enc(lengths, clip_n=[1, 0, 2]) == bad and enc(lengths, clip_n=[1, nc + 1, 2]) == bad
    assert frc([T, 0, 1]) == bad and b"frame_lengths[1]" in lib.escx_last_error()
    assert frc([T, 1, T + 1]) == bad and frc([T, 1, 1], clip_n=[1, 0, 2]) == bad
    assert dec([T, 0, 1]) == bad and b"frame_lengths[1]" in lib.escx_last_error()
    assert dec([T, 1, T + 1]) == bad and dec([T, 1, 1], caps=[4, 0, 4]) == bad
    assert lib.escx_dac_set_padding(hd, 0) == 0                                          # padding off
    assert enc(lengths) == bad and b"padding" in lib.escx_last_error()
    assert frc([T, 1, 1]) == bad and dec([T, 1, 1]) == bad
    assert lib.escx_dac_set_padding(hd, 1) == 0
    torch.cuda.synchronize()
    fresh = _new_model("dac_syn").set_precision(precision)
    for a, b in zip(m.encode(x, lengths=lengths), fresh.encode(x, lengths=lengths)):
        assert torch.equal(a, b)
    for a, b in zip(m.encode(x), fresh.encode(x)):                                       # and the plain entry point
        assert torch.equal(a, b)
    assert enc(lengths) == 0 and frc(m.frame_lengths(lengths).tolist()) == 0 and dec(m.frame_lengths(lengths).tolist()) == 0
    torch.cuda.synchronize()
