"""Per-clip n_quantizers and one-pass sweeps of the DAC baseline (esc.baselines.DAC) on the MI355X, in fp32 and bf16x3: a clip of a mixed
batch against the uniform call on that clip alone (bitwise), the ignored slots, the masked-mean losses, the real reference's codes for the
fixture clips, encode_sweep's snapshots against the uniform z (bitwise) and the reference's z, from_codes with counts, forward with counts
and the argument errors of the two C entry points (include/escx.h escx_dac_encode_ex, escx_dac_from_codes_ex)."""
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


def _x(pcm):
    return torch.from_numpy(synth.pcm_to_float(pcm))[:, None].cuda()


def _clips(name, n_samples, count, first=None):
    """`first` (fixture PCM rows) followed by synthesised noise / voiced clips up to `count` rows."""
    rows = [] if first is None else list(first)
    i = 0
    while len(rows) < count:
        rows.append((synth.voiced_clip_int16 if i % 2 else synth.noise_clip_int16)(f"dac-counts-{name}-{i}", n_samples))
        i += 1
    return _x(np.stack(rows))


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _check_per_clip(m, x, counts):
    """Every clip of encode(x, counts) against the uniform call on that clip alone; returns the mixed call's codes."""
    d = m.codebook_dim
    z, codes, lat, cm, cb = m.encode(x, counts)
    counts = [int(n) for n in counts]
    nmax = min(max(counts), m.n_codebooks)
    B, T = x.shape[0], z.shape[-1]
    assert z.shape == (B, m.latent_dim, T) and codes.shape == (B, nmax, T) and lat.shape == (B, nmax * d, T)
    assert codes.dtype == torch.int64 and cm.dim() == 0 and cb.dim() == 0
    solo_cm, solo_cb = [], []
    for b, n in enumerate(counts):
        n = min(n, m.n_codebooks)
        z1, c1, l1, cm1, cb1 = m.encode(x[b:b + 1], n)
        assert torch.equal(z[b:b + 1], z1), (b, n)
        assert torch.equal(codes[b:b + 1, :n], c1), (b, n)
        assert torch.equal(lat[b:b + 1, :n * d], l1), (b, n)
        assert bool((codes[b, n:] == -1).all()) and bool((lat[b, n * d:] == 0).all()), (b, n)
        solo_cm.append(float(cm1)); solo_cb.append(float(cb1))
    # sum_i mean_b(loss_ib [i < n_b]) (quantize.py:189-190) = mean_b of the clips' own sums
    print(f"losses {float(cm):.8g} {float(cb):.8g}  mean of the solo calls {np.mean(solo_cm):.8g} {np.mean(solo_cb):.8g}")
    np.testing.assert_allclose(float(cm), np.mean(solo_cm), rtol=1e-5)
    np.testing.assert_allclose(float(cb), np.mean(solo_cb), rtol=1e-5)
    return codes


@pytest.mark.parametrize("precision", PRECISIONS)
def test_per_clip_encode_syn(model, precision):
    """latent 32 (J = 1), 4 codebooks; 3 x 401 = 1203 rows: the last workgroup of four waves is ragged."""
    m = model("dac_syn", precision)
    g = load_golden("dac_syn")
    x = m.preprocess(_clips("dac_syn", 1603, 3, first=g["fwd_pcm"]), None)
    assert m.num_frames(x.shape[-1]) == 401
    _check_per_clip(m, x, [1, 4, 2])
    _check_per_clip(m, x, torch.tensor([4, 18, 3]))                      # a tensor; an entry above n_codebooks is clamped


@pytest.mark.parametrize("precision", PRECISIONS)
def test_per_clip_encode_tiny_and_the_reference_codes(model, precision):
    """latent 512 (J = 8), 18 codebooks.  The counts are all in the fixture's set, so the two fixture clips are also held to the real reference's
    codes under the near-tie rule."""
    m = model("dac_tiny", precision)
    g = load_golden("dac_tiny")
    counts = [1, 18, 6, 12]
    assert all(n in du.GOLDEN_NS for n in counts)
    x = _clips("dac_tiny", 16000, 4, first=g["pcm"])
    codes = _check_per_clip(m, x, counts).cpu().numpy()
    ref = None
    for b in range(g["pcm"].shape[0]):
        n = counts[b]
        got, want = codes[b:b + 1, :n], g[f"codes_{du.nkey(n)}"][b:b + 1].astype(np.int64)
        if np.array_equal(got, want):
            continue
        ref = ref or du.DacRef(_cfg("dac_tiny"), _sd("dac_tiny"))
        with torch.no_grad():
            z_enc = ref.encoder(x[b:b + 1].cpu())
        rows, bad = du.attribute_codes(ref, z_enc, n, got, want, g["margins"][b:b + 1, :n])
        assert not bad, f"clip {b}: codes differ beyond the near-tie rule: {bad[:5]}"


@pytest.mark.parametrize("precision", PRECISIONS)
def test_per_clip_encode_base(model, precision):
    """latent 1024 (J = 16)."""
    m = model("dac_base", precision)
    _check_per_clip(m, _clips("dac_base", 3200, 2), [2, 18])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,ns", [("dac_tiny", [1, 2, 6, 12, 18]), ("dac_syn", [1, 2, 4])])
def test_sweep_snapshots(model, precision, name, ns):
    m = model(name, precision)
    g = load_golden(name)
    x = _x(g["pcm"])
    zs, codes, lat = m.encode_sweep(x, ns)
    assert zs.shape == (len(ns), x.shape[0], m.latent_dim, m.num_frames(x.shape[-1]))
    for r, n in enumerate(ns):
        z, c, l, _, _ = m.encode(x, n)
        assert torch.equal(zs[r], z), n
    assert torch.equal(codes, c) and torch.equal(lat, l)                  # those of the largest count
    zs2, codes2, _ = m.encode_sweep(x, ns[-1:])                            # one snapshot: the final z itself
    assert torch.equal(zs2[0], zs[-1]) and torch.equal(codes2, codes)
    if name == "dac_syn":
        for r, key in enumerate(("z_n1", "z_n2", "z_nall")):
            err = _rel(zs[r].cpu(), g[key])
            print(f"{precision} {key}: max-relative {err:.3e}")
            assert err < 1e-5, key


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,n_samples,counts", [("dac_syn", 1603, [1, 4, 2]), ("dac_tiny", 16000, [1, 18, 6, 12])])
def test_from_codes_with_counts(model, precision, name, n_samples, counts):
    m = model(name, precision)
    d = m.codebook_dim
    x = m.preprocess(_clips(name, n_samples, len(counts)), None)
    codes = m.encode(x, counts)[1]                                         # -1 in the ignored slots
    z, zp, c = m.quantizer.from_codes(codes, counts)
    assert c is codes and zp.shape == (len(counts), codes.shape[1] * d, codes.shape[2])
    for b, n in enumerate(counts):
        z1, zp1, _ = m.quantizer.from_codes(codes[b:b + 1, :n])
        assert torch.equal(z[b:b + 1], z1) and torch.equal(zp[b:b + 1, :n * d], zp1), (b, n)
        assert bool((zp[b, n * d:] == 0).all()), (b, n)
    junk = codes.clone()
    for b, n in enumerate(counts):
        junk[b, n:] = torch.tensor([m.codebook_size + 5, -1, 2 ** 40, 3], device="cuda").repeat(codes.shape[2] // 4 + 1)[:codes.shape[2]]
    z2, zp2, _ = m.quantizer.from_codes(junk, torch.tensor(counts))
    assert torch.equal(z2, z) and torch.equal(zp2, zp)
    with pytest.raises(IndexError):
        m.quantizer.from_codes(codes)                                      # without counts a negative code still raises
    live = codes.clone(); live[0, 0, 0] = -1
    with pytest.raises(IndexError):
        m.quantizer.from_codes(live, counts)                               # a slot that is read is still checked
    with pytest.raises(ValueError):
        m.quantizer.from_codes(codes[:, :1], counts)                       # counts above the code slots


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,n_samples,counts", [("dac_syn", 1603, [1, 4, 2]), ("dac_tiny", 16123, [18, 1, 6])])
def test_forward_with_counts(model, precision, name, n_samples, counts):
    m = model(name, precision)
    x = _clips(name, n_samples, len(counts))
    out = m(x, None, counts)
    assert set(out) == {"audio", "z", "codes", "latents", "vq/commitment_loss", "vq/codebook_loss"}
    assert out["audio"].shape == (len(counts), 1, n_samples) and out["codes"].shape[1] == max(counts)
    for b, n in enumerate(counts):
        solo = m(x[b:b + 1], None, n)
        assert torch.equal(out["audio"][b:b + 1], solo["audio"]), (b, n)
        assert torch.equal(out["codes"][b:b + 1, :n], solo["codes"]), (b, n)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_c_abi_argument_errors_leave_the_handle_usable(model, precision):
    from esc import _native
    lib = _native.load()
    m = _new_model("dac_syn").set_precision(precision)
    x = m.preprocess(_clips("dac_syn", 1603, 3), None).contiguous()
    B, L, T, nc, d = 3, x.shape[-1], 401, m.n_codebooks, m.codebook_dim
    _, hd, flat, dev, stream = m._ctx(x, "x")
    z = torch.empty(B, m.latent_dim, T, device="cuda")
    zs = torch.empty(nc, B, m.latent_dim, T, device="cuda")
    codes = torch.zeros(B, nc, T, dtype=torch.int64, device="cuda")
    lat = torch.empty(B, nc * d, T, device="cuda")
    losses = torch.empty(2, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    arr = lambda v: (ctypes.c_int32 * len(v))(*v)         # noqa: E731

    def enc(n_q, clip_n, snap_n):
        return lib.escx_dac_encode_ex(hd, p(flat), m._version(), p(x), B, L, n_q, arr(clip_n) if clip_n else None, arr(snap_n) if snap_n else None,
                                      len(snap_n) if snap_n else 0, p(z), p(codes), p(lat), p(losses), p(zs), stream)

    def dec(n, clip_n):
        return lib.escx_dac_from_codes_ex(hd, p(flat), m._version(), p(codes), B, n, T, arr(clip_n), p(z), p(lat), stream)

    bad = _native.ESCX_ERR_INVALID_ARG
    assert enc(nc, [1, 0, 2], None) == bad                               # a count of 0
    assert enc(nc, [1, nc + 1, 2], None) == bad                          # a count above n_codebooks
    assert enc(2, [1, 4, 2], None) == bad                                # n_quantizers below max(clip_n)
    assert enc(nc, None, [2, 2]) == bad and enc(nc, None, [3, 1]) == bad # snapshots that do not increase
    assert enc(nc, None, [0, 1]) == bad and enc(2, None, [1, 3]) == bad  # ... or leave [1, n_quantizers]
    assert enc(nc, [1, 4, 2], [1, 2]) == bad                             # both inputs at once
    assert b"combined" in lib.escx_last_error()
    assert dec(nc, [1, 0, 2]) == bad and dec(nc, [1, nc + 1, 2]) == bad and dec(2, [1, 4, 2]) == bad
    torch.cuda.synchronize()
    got = m.encode(x, [1, 4, 2])
    sweep = m.encode_sweep(x, [1, 2, 4])
    fresh = _new_model("dac_syn").set_precision(precision)
    for a, b in zip(got + sweep, fresh.encode(x, [1, 4, 2]) + fresh.encode_sweep(x, [1, 2, 4])):
        assert torch.equal(a, b)
    assert torch.equal(m.encode(x, 3)[0], fresh.encode(x, 3)[0])         # and the plain entry point
