"""The DAC baseline's stand-alone quantiser on the MI355X (esc.baselines.DAC: model.quantizer(z, n_quantizers, frame_lengths) with its gradients
and model.quantizer.from_latents; include/escx.h escx_dac_quantize and its neighbours) against the REAL reference's fixture
(tools/gen_dac_quantizer_golden.py; every stored margin is at least 1e-5, so the codes must be equal, with no near-tie rule), the existing
dac_syn / dac_tiny / dac_base goldens, and the float64 restatement of tests/dac_quantizer_util.py that the host test pins to the fixture.

Shapes: dac_syn (D 32: one 64-channel register slice per lane, d 4, K 64, 4 stages), its variants latent_dim 96 / 192 (two / four slices) and
codebook_size 100 (K no multiple of 64), dac_tiny (D 512, d 8, K 1024, 18 stages), dac_base (D 1024).  3 x 7 frames are 21 rows: a ragged last
4-row workgroup; dac_base's 1 x 3 rows x 18 stages and the remainder slices give the search kernel wave counts that are no multiple of 4.

Gradients follow tests/test_dac_encode_grad.py's rule, err_dev <= 2 err_eager against float64 with the device's codes forced, err_eager being
float32 torch eager on the CPU; the parameters' follow tests/test_dac_encode_param_grad.py's per-kind rule.  EAGER holds the err_eager this
project measured on the CPU per case; the sanity window is a factor 10 on either side of it."""
import ctypes

import numpy as np
import pytest
import torch

import dac_quantizer_util as qu
from conftest import load_golden

eu, du, pu = qu.eu, qu.du, qu.pu
pytestmark = pytest.mark.gpu
TIE = 2e-6                                                  # dac_util.attribute_codes' threshold on a recorded margin
# err_eager of d_z on the CPU (float32 torch eager of the restatement against float64), per case
EAGER = {"dac_syn": 1.23e-7, "dac_syn:clip": 1.38e-7, "J2": 1.81e-7, "J4": 2.75e-7, "K100": 1.46e-7, "dac_tiny": 3.78e-7, "dac_tiny:clip": 3.30e-7,
         "dac_base": 4.46e-7}
_CACHE = {}


def _case(key):
    """(cfg, sd, model, z float32 numpy (B, D, T), n_codebooks) of a fixture configuration or of a dac_syn variant (seeded z, 3 x 7 frames)."""
    if key not in _CACHE:
        if key in qu.CASES:
            cfg, sd = eu.config(key), eu.state_dict(key)
            z = load_golden("dac_quantizer")[f"{key}_z"]
        else:
            cfg, sd = qu.variant(key)
            z = eu.seeded(f"quantizer-z:{key}", (3, du.full_config(cfg)["latent_dim"], 7)).astype(np.float32)
        _CACHE[key] = (cfg, sd, qu.model_of(cfg, sd), z, cfg["n_codebooks"])
    return _CACHE[key]


def _dev(a, dtype=np.float32):
    return torch.from_numpy(np.asarray(a, dtype)).cuda()


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _np(t):
    return t.detach().cpu().numpy()


def _param(m, key):
    return m.get_parameter(key)


def _same(a, b):
    return all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y) for x, y in zip(a, b))


def _against_restatement(key, out, z, n, counts=None):
    """z_q / latents within 1e-5 relative maximum and the losses within rtol 1e-5 of the float64 restatement continued from the device's codes:
    tests/test_dac.py's bounds for encode."""
    cfg, sd = _case(key)[:2]
    codes = _np(out[1])
    want = qu.run_ref(cfg, sd, z, n, torch.float64, codes=codes, counts=counts)
    assert _rel(_np(out[0]), want["z"]) < 1e-5 and _rel(_np(out[2]), want["latents"]) < 1e-5, key
    np.testing.assert_allclose([float(out[3]), float(out[4])], [want["cm"], want["cb"]], rtol=1e-5)


# ---- values ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(qu.CASES))
def test_values_against_the_reference_fixture(name):
    g = load_golden("dac_quantizer")
    cfg, sd, m, z, S = _case(name)
    d = cfg["codebook_dim"]
    zt = _dev(z)
    full = m.quantizer(zt)
    assert all(o.grad_fn is None and not o.requires_grad for o in full)
    assert full[1].dtype == torch.int64 and full[3].dim() == 0 and full[4].dim() == 0
    for nq in du.GOLDEN_NS:                                  # 18 is above dac_syn's 4 codebooks: it means 4
        k, ne = du.nkey(nq), S if nq is None else min(nq, S)
        zq, codes, lat, cm, cb = m.quantizer(zt, nq)
        assert tuple(codes.shape) == (z.shape[0], ne, z.shape[2]) and tuple(lat.shape) == (z.shape[0], ne * d, z.shape[2])
        np.testing.assert_array_equal(_np(codes), g[f"{name}_codes_{k}"].astype(np.int64))
        assert torch.equal(codes, full[1][:, :ne]) and torch.equal(lat, full[2][:, :ne * d]), "the codes and latents of a smaller n are a prefix"
        assert _rel(_np(lat), g[f"{name}_latents"][:, :ne * d]) < 1e-5, k
        np.testing.assert_allclose(float(cm), float(g[f"{name}_cm_{k}"]), rtol=1e-5)
        np.testing.assert_allclose(float(cb), float(g[f"{name}_cb_{k}"]), rtol=1e-5)
        if f"{name}_zq_{k}" in g.files:
            assert _rel(_np(zq), g[f"{name}_zq_{k}"]) < 1e-5, k
    counts = [int(c) for c in g[f"{name}_counts"]]
    zq, codes, lat, cm, cb = m.quantizer(zt, counts)
    n = max(counts)
    assert tuple(codes.shape) == (z.shape[0], n, z.shape[2])
    assert _rel(_np(zq), g[f"{name}_zq_clip"]) < 1e-5
    np.testing.assert_allclose(float(cm), float(g[f"{name}_cm_clip"]), rtol=1e-5)
    np.testing.assert_allclose(float(cb), float(g[f"{name}_cb_clip"]), rtol=1e-5)
    for b, nb in enumerate(counts):
        np.testing.assert_array_equal(_np(codes[b, :nb]), g[f"{name}_codes_nall"][b, :nb].astype(np.int64))
        assert bool((codes[b, nb:] == -1).all()) and not bool(lat[b, nb * d:].any())
    assert _same(m.quantizer(zt, torch.tensor(counts)), (zq, codes, lat, cm, cb))
    _against_restatement(name, full, z, None)


@pytest.mark.parametrize("which", sorted(qu.VARIANTS))
def test_values_of_the_other_kernel_paths_against_float64(which):
    cfg, sd, m, z, S = _case(which)
    ref = du.DacRef(cfg, sd)
    for n, counts in ((None, None), (3, None), (4, [2, 4, 1])):
        out = m.quantizer(_dev(z), n if counts is None else counts)
        want = ref.quantize(torch.from_numpy(z), n, margins=True)
        got = _np(out[1])
        if counts is None:
            rows, bad = du.attribute_codes(ref, torch.from_numpy(z), n, got, want[1].numpy(), want[5].numpy()) if not np.array_equal(got, want[1].numpy()) else (0, [])
            assert not bad, bad[:5]
        assert int(got.max()) < cfg["codebook_size"]
        _against_restatement(which, out, z, n, counts)


@pytest.mark.parametrize("key", ["dac_syn", "J2", "dac_tiny"])
def test_bitwise_invariants(key):
    cfg, sd, m, z, S = _case(key)
    d = cfg["codebook_dim"]
    B, _, T = z.shape
    zt = _dev(z)
    n = min(3, S)
    base = m.quantizer(zt, n)
    assert _same(m.quantizer(zt, n), base), "two calls differ"
    try:
        m.set_precision("bf16x3")
        assert _same(m.quantizer(zt, n), base), "the quantiser has no matrix-core operand: bf16x3 must not change it"
        m.set_precision("fp32")
        m.padding = False
        assert _same(m.quantizer(zt, n), base), "the quantiser has no convolution: the padding must not change it"
    finally:
        m.set_precision("fp32")
        m.padding = True
    counts = [(b % n) + 1 for b in range(B)]
    clip = m.quantizer(zt, counts)
    fl = [T - (2 * b) % T for b in range(B)]
    assert min(fl) >= 1 and (B == 1 or min(fl) < T)
    dead = torch.arange(T, device="cuda")[None, None, :] >= torch.tensor(fl, device="cuda")[:, None, None]
    lens = m.quantizer(zt, counts, frame_lengths=fl)
    poisoned = m.quantizer(torch.where(dead, torch.full_like(zt, float("nan")), zt), counts, frame_lengths=fl)
    assert _same(poisoned, lens), "something at or past a clip's length was read"
    cms, cbs = [], []
    for b in range(B):
        one = m.quantizer(zt[b:b + 1], n)
        assert all(torch.equal(one[i][0], base[i][b]) for i in range(3)), "a clip's result depends on its batch"
        nb, tb = counts[b], fl[b]
        own = m.quantizer(zt[b:b + 1], nb)
        assert torch.equal(own[0][0], clip[0][b]) and torch.equal(own[1][0], clip[1][b, :nb]) and torch.equal(own[2][0], clip[2][b, :nb * d])
        short = m.quantizer(zt[b:b + 1, :, :tb].contiguous(), nb)
        assert torch.equal(short[0][0], lens[0][b, :, :tb]) and torch.equal(short[1][0], lens[1][b, :nb, :tb]) and torch.equal(short[2][0], lens[2][b, :nb * d, :tb])
        assert not bool(lens[0][b, :, tb:].any()) and not bool(lens[2][b, :, tb:].any()) and bool((lens[1][b, :, tb:] == -1).all())
        assert bool((lens[1][b, nb:] == -1).all()) and not bool(lens[2][b, nb * d:].any())
        cms.append(float(short[3])); cbs.append(float(short[4]))
    np.testing.assert_allclose([float(lens[3]), float(lens[4])], [np.mean(cms), np.mean(cbs)], rtol=1e-6)


# ---- from_latents ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["dac_syn", "dac_tiny", "dac_base"])
def test_from_latents_against_the_encode_goldens(name):
    g = load_golden(name)
    m = _case(name)[2]
    lat, want, margins = g["latents"], g["codes_nall"].astype(np.int64), g["margins"]
    zq, zp, codes = m.quantizer.from_latents(_dev(lat))
    assert all(o.grad_fn is None and not o.requires_grad for o in (zq, zp, codes)) and codes.dtype == torch.int64
    got = _np(codes)
    differ = got != want
    assert got.shape == want.shape and bool((margins[differ] < TIE).all()), f"{int(differ.sum())} codes differ, margins {margins[differ][:5]}"
    fq, fp, _ = m.quantizer.from_codes(codes)
    assert torch.equal(zq, fq) and torch.equal(zp, fp), "(z_q, z_p) are not bitwise from_codes of the device's codes"
    if not differ.any():
        assert _rel(_np(zq), g["fc_z"]) < 1e-5
    print(f"{name}: {got.size} codes, {int(differ.sum())} differ at a recorded near-tie")


@pytest.mark.parametrize("key", ["dac_syn", "K100", "J4", "dac_tiny", "dac_base"])
def test_from_latents_returns_the_codes_of_the_quantiser(key):
    cfg, sd, m, z, S = _case(key)
    d = cfg["codebook_dim"]
    q = m.quantizer(_dev(z))
    zq, zp, codes = m.quantizer.from_latents(q[2])
    assert torch.equal(codes, q[1]), "from_latents(quantizer(z)[2])[2] is not quantizer(z)[1]"
    fq, fp, _ = m.quantizer.from_codes(codes)
    assert torch.equal(zq, fq) and torch.equal(zp, fp)
    if key in qu.CASES:
        g = load_golden("dac_quantizer")
        np.testing.assert_array_equal(_np(codes), g[f"{key}_fl_codes"].astype(np.int64))
        assert _rel(_np(zq), g[f"{key}_fl_zq"]) < 1e-5 and np.array_equal(_np(zp), g[f"{key}_fl_zp"])
        C = int(g[f"{key}_flr_channels"])                    # a remainder: C // d stages, and rows x stages no multiple of 4 for dac_syn
        rq, rp, rc = m.quantizer.from_latents(q[2][:, :C])
        np.testing.assert_array_equal(_np(rc), g[f"{key}_flr_codes"].astype(np.int64))
        assert tuple(rp.shape) == (z.shape[0], C // d * d, z.shape[2]) and _rel(_np(rq), g[f"{key}_flr_zq"]) < 1e-5
        junk = q[2][:, :C].clone()
        junk[:, C // d * d:] = float("nan")
        assert _same(m.quantizer.from_latents(junk), (rq, rp, rc)), "the channels that fill no codebook were read"
        assert _same(m.quantizer.from_latents(q[2][:, :C // d * d]), (rq, rp, rc))


def test_from_latents_of_an_encode_returns_its_codes():
    g = load_golden("dac_syn")
    m = _case("dac_syn")[2]
    from esc import synth
    x = torch.from_numpy(synth.pcm_to_float(g["pcm"]))[:, None, :402].cuda()
    z, codes, lat, _, _ = m.encode(x)
    assert torch.equal(m.quantizer.from_latents(lat)[2], codes)
    q = m.quantizer(z.flip(0).contiguous())                  # the quantiser alone on another latent still agrees with its own from_latents
    assert torch.equal(m.quantizer.from_latents(q[2])[2], q[1])


def test_from_latents_edges():
    cfg, sd = eu.config("dac_syn"), eu.state_dict("dac_syn")
    m = qu.model_of(cfg, sd)
    d, S, K = cfg["codebook_dim"], cfg["n_codebooks"], cfg["codebook_size"]
    with torch.no_grad():                                   # two identical codebook rows: the lower index wins
        cb1 = _param(m, f"quantizer.quantizers.{1}.codebook.weight")
        cb1[40].copy_(cb1[7])
    cb1 = cb1.detach()
    B, T = 2, 5
    lat = _dev(eu.seeded("quantizer-edges", (B, S * d, T)))
    lat[0, d:2 * d, 2] = cb1[7]
    lat[1, :, 3] = 0.0                                      # a zero latent: every distance is the codebook row's own norm
    lat[1, 2 * d:3 * d, 1] = float("nan")                   # every distance NaN: code 0
    zq, zp, codes = m.quantizer.from_latents(lat)
    assert int(codes[0, 1, 2]) == 7
    assert int(codes[1, 2, 1]) == 0
    assert int(codes.min()) >= 0 and int(codes.max()) < K
    for i in range(S):
        assert torch.equal(zp[1, i * d:(i + 1) * d, 3], _param(m, f"quantizer.quantizers.{i}.codebook.weight").detach()[codes[1, i, 3]])
    fq, fp, _ = m.quantizer.from_codes(codes)
    assert torch.equal(zq, fq) and torch.equal(zp, fp)
    assert _same(m.quantizer.from_latents(lat), (zq, zp, codes))
    # the count and length forms
    counts, fl = [2, 4], [5, 3]
    cq, cp, cc = m.quantizer.from_latents(lat, counts)
    for b, nb in enumerate(counts):
        assert torch.equal(cc[b, :nb], codes[b, :nb]) and bool((cc[b, nb:] == -1).all()) and not bool(cp[b, nb * d:].any())
        assert torch.equal(cq[b], m.quantizer.from_latents(lat[b:b + 1, :nb * d])[0][0])
    kq, kp, _ = m.quantizer.from_codes(cc, counts)
    assert torch.equal(cq, kq) and torch.equal(cp, kp)
    assert _same(m.quantizer.from_latents(lat, 2), m.quantizer.from_latents(lat, [2, 2]))
    poisoned = lat.clone()
    poisoned[1, :, 3:] = float("nan")
    lq, lp, lc = m.quantizer.from_latents(poisoned, counts, frame_lengths=fl)
    assert bool((lc[1, :, 3:] == -1).all()) and not bool(lq[1, :, 3:].any()) and not bool(lp[1, :, 3:].any())
    assert torch.equal(lc[0], cc[0]) and torch.equal(lq[0], cq[0]) and torch.equal(lc[1, :, :3], cc[1, :, :3]) and torch.equal(lq[1, :, :3], cq[1, :, :3])
    one = m.quantizer.from_latents(lat[1:2, :, :3].contiguous())
    assert torch.equal(one[2][0], lc[1, :, :3]) and torch.equal(one[0][0], lq[1, :, :3])
    assert not any(o.requires_grad for o in m.quantizer.from_latents(lat.clone().requires_grad_(True)))


# ---- d_z ------------------------------------------------------------------------------------------------------------------------------------
def _cot(key, z, n, d, per_clip=False):
    if key in qu.CASES:
        c = qu.cotangents(key, per_clip)
    else:
        B, D, T = z.shape
        c = {"z": eu.seeded(f"w_zq:{key}", (B, D, T)), "latents": eu.seeded(f"w_lat:{key}", (B, n * d, T)), "cm": np.float64(np.float32(0.8 * d * T)),
             "cb": np.float64(np.float32(0.7 * d * T))}
    return c


def _check_dz(key, tag, dz, z, cot, n, codes, counts, d64=None):
    cfg, sd = _case(key)[:2]
    if d64 is None:
        d64 = qu.grads(cfg, sd, z, cot, n, codes=codes, counts=counts)[0]
    err_eager = eu.rel_l2(qu.grads(cfg, sd, z, cot, n, torch.float32, codes=codes, counts=counts)[0], d64)
    err_dev = eu.rel_l2(_np(dz), d64)
    print(f"{tag}: err_dev {err_dev:.3e}  err_eager {err_eager:.3e}  ratio {err_dev / err_eager:.2f}")
    assert EAGER[tag] / 10 < err_eager < EAGER[tag] * 10, (tag, err_eager)
    assert dz.dtype == torch.float32 and err_dev <= 2 * err_eager, (tag, err_dev, err_eager)


@pytest.mark.parametrize("key", ["dac_syn", "J2", "J4", "K100", "dac_tiny", "dac_base"])
def test_latent_gradient_against_float64(key):
    cfg, sd, m, z, S = _case(key)
    d = cfg["codebook_dim"]
    cot = {k: v for k, v in _cot(key, z, S, d).items() if k != "cb"}
    out, dz, _ = qu.device_grads(m, z, cot, None)
    zq, codes, lat, cm, cb = out
    assert zq.grad_fn is not None and lat.grad_fn is not None and cm.grad_fn is not None and not codes.requires_grad and not cb.requires_grad
    with torch.no_grad():
        assert _same(tuple(o.detach() for o in out), m.quantizer(_dev(z))), "the grad path's values are not bitwise the plain call's"
    d64 = None
    if key in qu.CASES:
        g = load_golden("dac_quantizer")
        np.testing.assert_array_equal(_np(codes), g[f"{key}_codes_nall"].astype(np.int64))
        d64 = g[f"{key}_d_z"]
    _check_dz(key, key, dz, z, cot, None, _np(codes), None, d64)
    for k in cot:                                           # each of the three differentiable outputs on its own reaches z
        _, part, _ = qu.device_grads(m, z, {k: cot[k]}, None)
        want = qu.grads(cfg, sd, z, {k: cot[k]}, None, codes=_np(codes))[0]
        assert eu.rel_l2(_np(part), want) < 1e-5, k
    with pytest.raises(RuntimeError):                       # first order only
        zt = _dev(z).requires_grad_(True)
        o = m.quantizer(zt)
        gz, = torch.autograd.grad(o[0].sum(), zt, create_graph=True)
        gz.sum().backward()


@pytest.mark.parametrize("name", ["dac_syn", "dac_tiny"])
def test_latent_gradient_with_per_clip_counts(name):
    g = load_golden("dac_quantizer")
    cfg, sd, m, z, S = _case(name)
    d = cfg["codebook_dim"]
    B, D, T = z.shape
    counts = [int(c) for c in g[f"{name}_counts"]]
    n = max(counts)
    cot = {k: v for k, v in qu.cotangents(name, per_clip=True).items() if k != "cb"}
    cot["latents"] = cot["latents"][:, :n * d]
    out, dz, _ = qu.device_grads(m, z, cot, counts)
    codes = _np(out[1])
    forced = np.where(codes < 0, 0, codes)
    d64 = g[f"{name}_d_z_clip"] if name == "dac_syn" and n == S else None
    _check_dz(name, f"{name}:clip", dz, z, cot, n, forced, counts, d64)
    _, dz2, _ = qu.device_grads(m, z, cot, counts)
    assert torch.equal(dz, dz2), "two backwards differ"
    # a clip whose count is below n: the later stages' cotangents give exact zeros
    b = int(np.argmin(counts))
    assert counts[b] < n
    w = np.zeros((B, n * d, T))
    w[b, counts[b] * d:] = cot["latents"][b, counts[b] * d:]
    _, late, _ = qu.device_grads(m, z, {"latents": w}, counts)
    assert not bool(late.any()), "a stage past a clip's count reached z"
    # batch independence (no commitment cotangent: its mean runs over the batch)
    two = {k: cot[k] for k in ("z", "latents")}
    _, dzb, _ = qu.device_grads(m, z, two, counts)
    for b, nb in enumerate(counts):
        _, one, _ = qu.device_grads(m, z[b:b + 1], {"z": two["z"][b:b + 1], "latents": two["latents"][b:b + 1, :nb * d]}, nb)
        assert torch.equal(one[0], dzb[b]), "a clip's gradient depends on its batch"


def test_gradient_refusals_and_the_changed_parameter():
    cfg, sd = eu.config("dac_syn"), eu.state_dict("dac_syn")
    m = qu.model_of(cfg, sd)
    z = _dev(_case("dac_syn")[3]).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="frame_lengths"):
        m.quantizer(z, None, frame_lengths=[7, 3, 1])
    with torch.no_grad():
        assert m.quantizer(z, None, frame_lengths=[7, 3, 1])[0].grad_fn is None
    out = m.quantizer(z)
    with torch.no_grad():
        _param(m, f"quantizer.quantizers.{0}.out_proj.bias").add_(1.0)
    with pytest.raises(RuntimeError, match="changed in place"):
        out[0].sum().backward()
    assert z.grad is None
    m.set_encode_trainable("quantizer")
    for p in m.parameters():
        p.requires_grad_(True)
    with pytest.raises(NotImplementedError, match="frame_lengths"):
        m.quantizer(z.detach(), None, frame_lengths=[7, 3, 1])
    out = m.quantizer(z)
    with torch.no_grad():
        _param(m, f"quantizer.quantizers.{1}.codebook.weight").mul_(0.5)
    with pytest.raises(RuntimeError, match="changed in place"):
        (out[0].sum() + out[4]).backward()
    assert all(p.grad is None for p in m.parameters())
    out = m.quantizer(z)                                    # and the next good call succeeds
    (out[0].sum() + out[4]).backward()
    assert z.grad is not None and _param(m, f"quantizer.quantizers.{1}.codebook.weight").grad is not None


# ---- parameter gradients --------------------------------------------------------------------------------------------------------------------
def _trainable(key, part="quantizer"):
    cfg, sd = _case(key)[:2]
    m = qu.model_of(cfg, sd).set_encode_trainable(part)
    for p in m.parameters():
        p.requires_grad_(True)
    return m


@pytest.mark.parametrize("key,counts", [("dac_syn", None), ("dac_syn", "fixture"), ("J2", None), ("K100", [2, 3, 1]), ("dac_tiny", None)])
def test_parameter_gradients_against_float64(key, counts):
    cfg, sd, frozen, z, S = _case(key)
    d = cfg["codebook_dim"]
    if counts == "fixture":
        counts = [int(c) for c in load_golden("dac_quantizer")[f"{key}_counts"]]
    n = S if counts is None else max(counts)
    cot = _cot(key, z, S, d, per_clip=counts is not None)
    cot["latents"] = cot["latents"][:, :n * d]
    keys = qu.quantizer_keys(sd)
    m = _trainable(key)
    out, dz, grads = qu.device_grads(m, z, cot, counts, keys)
    assert out[4].requires_grad and not out[1].requires_grad
    with torch.no_grad():
        assert _same(tuple(o.detach() for o in out), frozen.quantizer(_dev(z), counts)), "the parameter path's values are not bitwise the plain call's"
    _, dz_frozen, _ = qu.device_grads(frozen, z, {k: v for k, v in cot.items() if k != "cb"}, counts)
    assert torch.equal(dz, dz_frozen), "z.grad differs between the parameter path and the frozen path"
    assert all(p.grad is None for k, p in m.named_parameters() if not k.startswith("quantizer."))
    codes = _np(out[1])
    forced = np.where(codes < 0, 0, codes)
    _, g64 = qu.grads(cfg, sd, z, cot, n, codes=forced, counts=counts, params=True)
    if key == "dac_syn" and counts is None:
        g = load_golden("dac_quantizer")
        np.testing.assert_array_equal(codes, g[f"{key}_codes_nall"].astype(np.int64))
        g64 = {k: g[f"{key}_g/{k}"] for k in keys}
    _, eager = qu.grads(cfg, sd, z, cot, n, torch.float32, codes=forced, counts=counts, params=True)
    assert [k for k in keys if grads[k] is None] == [k for k in keys if g64[k] is None] == [k for k in keys if pu.stage_of(k) >= n]
    ran = {k: v for k, v in g64.items() if v is not None}
    pu.check_rule(pu.errors(grads, ran), pu.errors(eager, ran), f"{key} counts {counts}")


def test_parameter_gradients_unrun_stages_accumulation_and_the_switch():
    cfg, sd, frozen, z, S = _case("dac_syn")
    d = cfg["codebook_dim"]
    keys = qu.quantizer_keys(sd)
    cot = _cot("dac_syn", z, S, d)
    cot["latents"] = cot["latents"][:, :2 * d]
    m = _trainable("dac_syn", "both")
    out, dz, once = qu.device_grads(m, z, cot, 2, keys)
    assert all((once[k] is None) == (pu.stage_of(k) >= 2) for k in keys), "not exactly the stages the call ran got a gradient"
    assert all(p.grad is None for k, p in m.named_parameters() if not k.startswith("quantizer."))
    named = dict(m.named_parameters())
    zt = _dev(z).requires_grad_(True)
    for p in m.parameters():
        p.grad = None
    for _ in range(2):                                      # two accumulated backwards are exactly twice one
        o = m.quantizer(zt, 2)
        (sum((t * _dev(cot[k])).sum() for k, t in (("z", o[0]), ("latents", o[2]))) + o[3] * float(cot["cm"]) + o[4] * float(cot["cb"])).backward()
    for k in keys:
        if once[k] is not None:
            assert np.array_equal(named[k].grad.double().cpu().numpy(), 2 * once[k]), k
    assert torch.equal(zt.grad, 2 * dz)
    # the encoder's switch alone gives the stand-alone call no parameter gradients; z still gets its own
    m.set_encode_trainable("encoder")
    for p in m.parameters():
        p.grad = None
    o, dz2, _ = qu.device_grads(m, z, {k: v for k, v in cot.items() if k != "cb"}, 2)
    assert not o[4].requires_grad and torch.equal(dz2, dz) and all(p.grad is None for p in m.parameters())
    # only the parameters that require a gradient get one
    m.set_encode_trainable("quantizer")
    for k, p in m.named_parameters():
        p.requires_grad_(k.endswith("codebook.weight"))
    _, _, some = qu.device_grads(m, z, cot, 2, keys)
    assert all((some[k] is not None) == (k.endswith("codebook.weight") and pu.stage_of(k) < 2) for k in keys)
    assert all(np.array_equal(some[k], once[k]) for k in keys if some[k] is not None)


# ---- C ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_c_abi_bad_arguments_leave_the_handle_usable():
    from esc import _native
    cfg, sd, m, z, S = _case("dac_syn")
    d = cfg["codebook_dim"]
    B, D, T = z.shape
    zt = _dev(z)
    want = m.quantizer(zt)
    lib, hd, flat, dev, stream = m._ctx(zt, "z")
    P = lambda t: ctypes.c_void_p(t.data_ptr())             # noqa: E731
    I = lambda v: (ctypes.c_int32 * len(v))(*v)             # noqa: E731
    zq, codes, lat, losses = torch.empty_like(zt), torch.empty(B, S, T, dtype=torch.int64, device="cuda"), torch.empty(B, S * d, T, device="cuda"), torch.empty(2, device="cuda")
    head = (hd, P(flat), m._version())
    outs = (P(zq), P(codes), P(lat), P(losses), stream)
    INV = _native.ESCX_ERR_INVALID_ARG
    assert lib.escx_dac_quantize(*head, P(zt), B, T, 0, *outs) == INV
    assert lib.escx_dac_quantize(*head, P(zt), B, 0, S, *outs) == INV
    assert lib.escx_dac_quantize(*head, None, B, T, S, *outs) == INV
    assert lib.escx_dac_quantize_ex(*head, P(zt), B, T, S, I([1, S + 1, 1]), *outs) == INV
    assert lib.escx_dac_quantize_ex(*head, P(zt), B, T, 2, I([1, 3, 1]), *outs) == INV
    assert lib.escx_dac_quantize_lengths(*head, P(zt), B, T, I([1, T + 1, 1]), S, None, *outs) == INV
    assert lib.escx_dac_quantize_lengths(*head, P(zt), B, T, None, S, None, *outs) == INV
    assert b"frame_lengths" in lib.escx_last_error()
    dz = torch.empty_like(zt)
    assert lib.escx_dac_quantize_backward(*head, P(want[2]), P(want[1]), B, T, 0, None, P(zt), None, None, P(dz), stream) == INV
    assert lib.escx_dac_quantize_backward(*head, P(want[2]), P(want[1]), B, T, S, None, P(zt), None, None, None, stream) == INV
    grad = torch.empty_like(flat)
    assert lib.escx_dac_quantize_backward_params(*head, None, P(want[2]), P(want[1]), B, T, S, None, P(zt), None, None, None, P(dz), P(grad), stream) == INV
    assert lib.escx_dac_quantize_backward_params(*head, P(zt), P(want[2]), P(want[1]), B, T, S, I([1, 0, 1]), P(zt), None, None, None, P(dz), P(grad), stream) == INV
    fz, fp, fc = torch.empty_like(zt), torch.empty(B, S * d, T, device="cuda"), torch.empty(B, S, T, dtype=torch.int64, device="cuda")
    assert lib.escx_dac_from_latents(*head, P(want[2]), B, d - 1, T, P(fz), P(fp), P(fc), stream) == INV
    assert lib.escx_dac_from_latents_ex(*head, P(want[2]), B, 2 * d, T, I([1, 3, 1]), P(fz), P(fp), P(fc), stream) == INV
    assert lib.escx_dac_from_latents_lengths(*head, P(want[2]), B, S * d, T, I([0, 1, 1]), None, P(fz), P(fp), P(fc), stream) == INV
    # the next good calls succeed and give the Python surface's bits
    assert lib.escx_dac_quantize(*head, P(zt), B, T, S, *outs) == 0
    assert lib.escx_dac_from_latents(*head, P(lat), B, S * d, T, P(fz), P(fp), P(fc), stream) == 0
    assert lib.escx_dac_quantize_backward(*head, P(lat), P(codes), B, T, S, None, P(zt), None, None, P(dz), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(zq, want[0]) and torch.equal(codes, want[1]) and torch.equal(lat, want[2]) and float(losses[0]) == float(want[3])
    assert torch.equal(fc, codes) and torch.equal(fz, m.quantizer.from_codes(codes)[0])
    ztg = zt.clone().requires_grad_(True)
    (m.quantizer(ztg)[0] * zt).sum().backward()
    assert torch.equal(ztg.grad, dz)
