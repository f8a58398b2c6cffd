"""CPU-side checks of the DAC baseline's stand-alone quantiser (esc.baselines.DAC: model.quantizer(z) and model.quantizer.from_latents): the two
methods exist with the reference's signature defaults, the refusals and argument errors come before anything touches a device, the library
exports and binds the new entry points and the header cites the reference for each, and the float64 restatement of
tests/dac_quantizer_util.py reproduces the REAL reference's fixture (tools/gen_dac_quantizer_golden.py).  No GPU here."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dac_quantizer_util as qu
from conftest import ROOT, load_golden

eu, du = qu.eu, qu.du
NEW_SYMBOLS = ("escx_dac_quantize", "escx_dac_quantize_ex", "escx_dac_quantize_lengths", "escx_dac_quantize_backward", "escx_dac_quantize_backward_params",
               "escx_dac_from_latents", "escx_dac_from_latents_ex", "escx_dac_from_latents_lengths")


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _model(train=False):
    from esc.baselines import DAC
    m = DAC(**eu.config("dac_syn"))
    return m.train() if train else m.eval()


def test_library_exports_binds_and_documents_the_quantiser_entry_points():
    from esc import _native
    lib = _native.load()
    header = open(os.path.join(ROOT, "include", "escx.h")).read()
    for name in NEW_SYMBOLS:
        assert name in _native.SIGNATURES, name
        fn = getattr(lib, name)
        restype, argtypes = _native.SIGNATURES[name]
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
        # the comment in front of the declaration cites the reference lines the entry point replaces
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", header, re.S)
        assert m and re.search(r"quantize\.py:\d+-\d+", m.group(1)), name


def test_the_quantizer_has_the_reference_surface():
    q = _model().quantizer
    assert callable(q) and callable(q.from_latents) and callable(q.from_codes)
    sig = inspect.signature(q.forward)
    assert list(sig.parameters) == ["z", "n_quantizers", "frame_lengths"]
    assert sig.parameters["n_quantizers"].default is None and sig.parameters["frame_lengths"].default is None
    sig = inspect.signature(q.from_latents)
    assert list(sig.parameters) == ["latents", "n_quantizers", "frame_lengths"]
    assert sig.parameters["n_quantizers"].default is None and sig.parameters["frame_lengths"].default is None
    assert "parameter gradients through from_latents are not built" in q.from_latents.__doc__


def test_refusals_and_argument_errors_come_before_the_device():
    m = _model()
    D, d, S = m.latent_dim, m.codebook_dim, m.n_codebooks
    z, lat = torch.zeros(2, D, 3), torch.zeros(2, S * d, 3)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.quantizer(z)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.quantizer(z, [1, 2], frame_lengths=[3, 1])
    with pytest.raises(RuntimeError, match="HIP device"):
        m.quantizer.from_latents(lat)
    for bad in (torch.zeros(2, D + 1, 3), torch.zeros(2, D, 0), torch.zeros(2, D), torch.zeros(0, D, 3)):
        with pytest.raises(ValueError, match="z must be"):
            m.quantizer(bad)
    for n in (0, -1, [0, 1], [1, 2, 3], [1]):
        with pytest.raises(ValueError):
            m.quantizer(z, n)
    for fl in ([0, 1], [1, 4], [1], [1, 2, 3]):
        with pytest.raises(ValueError, match="frame_lengths"):
            m.quantizer(z, None, fl)
        with pytest.raises(ValueError, match="frame_lengths"):
            m.quantizer.from_latents(lat, None, fl)
    with pytest.raises(ValueError, match="hold no codebook"):
        m.quantizer.from_latents(torch.zeros(2, d - 1, 3))
    with pytest.raises(ValueError, match="latents must be"):
        m.quantizer.from_latents(torch.zeros(2, d, 0))
    for n in (0, [0, 1], [1, 2, 3]):
        with pytest.raises(ValueError):
            m.quantizer.from_latents(lat, n)
    with pytest.raises(ValueError, match="for latents of 2 codebooks"):
        m.quantizer.from_latents(lat[:, :2 * d + 1], [3, 1])
    # frame_lengths together with a gradient is refused behind the device check (tests/test_dac_quantizer.py shows it on the GPU): a CPU tensor
    # is refused first, and nothing is differentiated
    zg = z.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.quantizer(zg, None, [1, 2])
    assert zg.grad is None


def test_training_mode_refuses():
    m = _model(train=True)
    z = torch.zeros(1, m.latent_dim, 2, requires_grad=True)
    with pytest.raises(NotImplementedError, match="inference only"):
        m.quantizer(z)
    with pytest.raises(NotImplementedError, match="inference only"):
        m.quantizer.from_latents(torch.zeros(1, m.codebook_dim, 2))
    assert z.grad is None


@pytest.mark.parametrize("name", sorted(qu.CASES))
def test_float64_restatement_reproduces_the_reference_fixture(name):
    """The bound is tests/test_dac_encode_grad_host.py's for its fixture: 1e-12 relative on the float64 gradients.  The forward values are
    stored in float32 and a float32 matrix product rounds differently at another thread count, so the float32 restatement is compared with
    them at tests/test_dac.py's bounds for encode (1e-5 relative maximum, rtol 1e-5 on the losses); the codes are exact (every margin is at
    least 1e-5)."""
    g = load_golden("dac_quantizer")
    cfg, sd = eu.config(name), eu.state_dict(name)
    B, T, n = qu.CASES[name]
    d = cfg["codebook_dim"]
    z, codes = g[f"{name}_z"], g[f"{name}_codes_nall"].astype(np.int64)
    assert z.dtype == np.float32 and z.shape == (B, du.full_config(cfg)["latent_dim"], T) and codes.shape == (B, n, T)
    assert float(g[f"{name}_margins"].min()) >= qu.MIN_MARGIN
    for nq in du.GOLDEN_NS:
        k, ne = du.nkey(nq), n if nq is None else min(nq, n)
        out = qu.run_ref(cfg, sd, z, nq, torch.float32)
        assert np.array_equal(out["codes"], g[f"{name}_codes_{k}"]) and np.array_equal(out["codes"], codes[:, :ne])
        assert _rel(out["latents"], g[f"{name}_latents"][:, :ne * d]) < 1e-5
        np.testing.assert_allclose([out["cm"], out["cb"]], [g[f"{name}_cm_{k}"], g[f"{name}_cb_{k}"]], rtol=1e-5)
        if f"{name}_zq_{k}" in g.files:
            assert _rel(out["z"], g[f"{name}_zq_{k}"]) < 1e-5
    counts = g[f"{name}_counts"]
    out = qu.run_ref(cfg, sd, z, None, torch.float32, counts=counts)
    assert _rel(out["z"], g[f"{name}_zq_clip"]) < 1e-5
    np.testing.assert_allclose([out["cm"], out["cb"]], [g[f"{name}_cm_clip"], g[f"{name}_cb_clip"]], rtol=1e-5)
    # from_latents' contract in the reference itself: the codes of forward, from_codes' sums
    ref = du.DacRef(cfg, sd)
    assert np.array_equal(g[f"{name}_fl_codes"], codes)
    fz, fzp, _ = ref.from_codes(torch.from_numpy(codes))
    assert _rel(fz.numpy(), g[f"{name}_fl_zq"]) < 1e-5 and np.array_equal(fzp.numpy(), g[f"{name}_fl_zp"])
    C = int(g[f"{name}_flr_channels"])
    assert C % d and np.array_equal(g[f"{name}_flr_codes"], codes[:, :C // d])
    assert _rel(ref.from_codes(torch.from_numpy(codes[:, :C // d]))[0].numpy(), g[f"{name}_flr_zq"]) < 1e-5
    # float64 autograd
    cot = qu.cotangents(name)
    d_z, grads = qu.grads(cfg, sd, z, cot, None, params=(name == "dac_syn"))
    forced, _ = qu.grads(cfg, sd, z, cot, None, codes=codes)
    err, errf = eu.rel_l2(d_z, g[f"{name}_d_z"]), eu.rel_l2(forced, g[f"{name}_d_z"])
    print(f"{name}: float64 restatement d_z vs reference {err:.3e} (codes forced {errf:.3e})")
    assert err <= 1e-12 and errf <= 1e-12
    for k in cot:                                           # every cotangent but the codebook loss' reaches z
        part = np.linalg.norm(qu.grads(cfg, sd, z, {k: cot[k]}, None)[0]) if k != "cb" else None
        assert part is None or part > 1e-3, k
    if name == "dac_syn":
        assert sorted(grads) == sorted(qu.quantizer_keys(sd))
        for k, v in grads.items():
            assert eu.rel_l2(v, g[f"{name}_g/{k}"]) <= 1e-12, k
        dzc, _ = qu.grads(cfg, sd, z, qu.cotangents(name, per_clip=True), None, counts=counts)
        assert eu.rel_l2(dzc, g[f"{name}_d_z_clip"]) <= 1e-12
