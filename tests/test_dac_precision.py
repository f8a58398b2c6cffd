"""The exact split-operand mode of the DAC baseline codec (DAC.set_precision("bf16x3"), include/escx.h escx_dac_set_precision): the host and C-ABI
contract, the untouched fp32 default, parity with the real reference's fixtures at the tolerances of tests/test_dac.py with every code exact,
the error against float64 next to the fp32 forms, the invariants of the fp32 path (batch independence, prefix property, Snake placement,
in-place parameter changes, also across a mode switch) and every branch of the new launcher."""
import contextlib
import json
import os
import re

import numpy as np
import pytest
import torch

import dac_util as du
from conftest import ROOT, load_golden, load_manifest
from esc import synth

gpu = pytest.mark.gpu
NAMES = ("dac_syn", "dac_tiny", "dac_base")
_MODELS = {}


def _cfg(name):
    return json.loads(str(load_golden(name)["config_json"]))


def _sd(name):
    return {k: torch.from_numpy(v) for k, v in synth.dac_state_dict(load_manifest(name)).items()}


def _fresh(name):
    from esc.baselines import DAC
    m = DAC(**_cfg(name))
    m.load_state_dict(_sd(name), strict=True)
    return m.cuda().eval()


def _model(name):
    if name not in _MODELS:
        _MODELS[name] = _fresh(name)
    return _MODELS[name]


@contextlib.contextmanager
def _mode(m, mode):
    """The shared models are in fp32 outside this block."""
    m.set_precision(mode)
    try:
        yield m
    finally:
        m.set_precision("fp32")


def _x(pcm):
    return torch.from_numpy(synth.pcm_to_float(pcm))[:, None].cuda()


def _clips(tag, n, L):
    return np.stack([synth.voiced_clip_int16(f"{tag}-{i}", L) if i % 2 else synth.noise_clip_int16(f"{tag}-{i}", L) for i in range(n)])


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def _rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean()) / max(np.sqrt((b ** 2).mean()), 1e-30))


# ---- 1. host contract, no device -----------------------------------------------------------------------------------------------------------
def test_precision_contract_on_host():
    from esc import _native
    from esc.baselines import DAC
    m = DAC(**_cfg("dac_syn"))
    assert m.precision == "fp32"
    assert m.set_precision("bf16x3") is m and m.precision == "bf16x3"
    assert m.set_precision("fp32").precision == "fp32"
    with pytest.raises(ValueError, match="precision"):
        m.set_precision("nope")
    with pytest.raises(NotImplementedError, match="Snake"):
        m.set_precision("f16x2")
    assert m.precision == "fp32"                                    # a refused mode changes nothing
    header = open(os.path.join(ROOT, "include", "escx.h")).read()
    lib = _native.load()
    for sym in ("escx_dac_set_precision", "escx_dac_get_precision"):
        assert re.search(rf"\bint {sym}\s*\(", header), sym
        assert sym in _native.SIGNATURES and hasattr(lib, sym), sym


# ---- 2. C ABI ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_abi_set_get_and_refusals():
    from esc import _native
    lib = _native.load()
    m = _fresh("dac_syn")
    _, hd = m._handle(torch.device("cuda:0"))
    assert lib.escx_dac_get_precision(hd) == _native.PRECISIONS["fp32"] == 0
    assert lib.escx_dac_set_precision(hd, _native.PRECISIONS["bf16x3"]) == 0 and lib.escx_dac_get_precision(hd) == 3
    assert lib.escx_dac_set_precision(hd, _native.PRECISIONS["f16x2"]) == _native.ESCX_ERR_UNSUPPORTED
    assert b"Snake" in lib.escx_last_error() and b"f16x2" in lib.escx_last_error()
    assert lib.escx_dac_set_precision(hd, 7) == _native.ESCX_ERR_INVALID_ARG
    assert lib.escx_dac_get_precision(hd) == 3                      # refusals leave the mode alone
    assert lib.escx_dac_set_precision(hd, 0) == 0 and lib.escx_dac_get_precision(hd) == 0
    assert lib.escx_dac_set_precision(None, 0) == _native.ESCX_ERR_INVALID_ARG and lib.escx_dac_get_precision(None) == -1
    m2 = _fresh("dac_syn").set_precision("bf16x3")                  # remembered before a handle exists, applied at creation
    m2b = type(m2)(**_cfg("dac_syn")).set_precision("bf16x3").cuda().eval()
    for mm in (m2, m2b):
        assert lib.escx_dac_get_precision(mm._handle(torch.device("cuda:0"))[1]) == 3 and mm.precision == "bf16x3"


# ---- 3. the default is untouched -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ("dac_syn", "dac_tiny"))
def test_fp32_after_a_round_trip_is_bitwise_a_fresh_model(name):
    g = load_golden(name)
    x, x2 = _x(g["pcm"]), _x(g["fwd_pcm"])
    a = _fresh(name)
    want_e = a.encode(x)
    want_d = a.decode(want_e[0])
    want_f = a(x2)
    b = _fresh(name).set_precision("bf16x3")
    b.encode(x), b.decode(want_e[0])                                # the split image exists and has been used
    b.set_precision("fp32")
    got_e = b.encode(x)
    for u, v in zip(got_e, want_e):
        assert torch.equal(u, v)
    assert torch.equal(b.decode(want_e[0]), want_d)
    got_f = b(x2)
    for k in want_f:
        assert torch.equal(got_f[k], want_f[k]), k


# ---- 4. reference parity in bf16x3 ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", NAMES)
def test_bf16x3_against_the_reference(name):
    """tests/test_dac.py's tolerances; every code must equal the reference's (the smallest reference margins of these fixtures are 4.6e-5, 4.3e-6
    and 6.9e-4, above the near-tie rule's 2e-6, so the rule excuses nothing here)."""
    g = load_golden(name)
    with _mode(_model(name), "bf16x3") as m:
        x = _x(g["pcm"])
        for n in du.GOLDEN_NS:
            k = du.nkey(n)
            z, codes, lat, cm, cb = m.encode(x, n)
            np.testing.assert_array_equal(codes.cpu().numpy(), g[f"codes_{k}"], err_msg=k)
            print(f"{name} {k}: latents {_rel(lat.cpu(), g['latents'][:, :lat.shape[1]]):.3g}")
            assert _rel(lat.cpu(), g["latents"][:, :lat.shape[1]]) < 1e-5, k
            np.testing.assert_allclose(float(cm), float(g[f"cm_{k}"]), rtol=1e-5)
            np.testing.assert_allclose(float(cb), float(g[f"cb_{k}"]), rtol=1e-5)
            if f"z_{k}" in g:
                assert _rel(z.cpu(), g[f"z_{k}"]) < 1e-5, k
            if f"audio_{k}" in g:
                a = m.decode(z).cpu().numpy()
                assert a.shape == g[f"audio_{k}"].shape
                print(f"{name} {k}: audio {_rel_rms(a, g[f'audio_{k}']):.3g}")
                assert _rel_rms(a, g[f"audio_{k}"]) < 1e-4, k
        zq, zp, _ = m.quantizer.from_codes(torch.from_numpy(g["codes_nall"].astype(np.int64)).cuda())
        assert _rel(zq.cpu(), g["fc_z"]) < 1e-5
        assert _rel_rms(m.decode(zq).cpu(), g["audio_nall"]) < 1e-4
        out = m(_x(g["fwd_pcm"]))
        np.testing.assert_array_equal(out["codes"].cpu().numpy(), g["fwd_codes"])
        assert out["audio"].shape[-1] == g["fwd_pcm"].shape[-1]
        assert _rel_rms(out["audio"].cpu(), g["fwd_audio"]) < 1e-4
        np.testing.assert_allclose(float(out["vq/commitment_loss"]), float(g["fwd_cm"]), rtol=1e-5)


# ---- 5. the mode is not a no-op ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ("dac_tiny", "dac_base"))
def test_bf16x3_is_another_arithmetic(name):
    m = _model(name)
    x = _x(load_golden(name)["pcm"])
    z32 = m.encode(x)[0]
    a32 = m.decode(z32)
    with _mode(m, "bf16x3"):
        z3 = m.encode(x)[0]
        a3 = m.decode(z32)
    assert not torch.equal(z3, z32) and not torch.equal(a3, a32)


# ---- 6. fp32-grade, measured ---------------------------------------------------------------------------------------------------------------
@gpu
def test_bf16x3_error_against_float64_is_fp32_grade():
    """dac_tiny, B = 2, against the restatement in float64 (float64 weights and input, CPU).  The encoder output is observable through the first
    quantiser stage's latents (in_proj of the encoder output, the same fp32 code in both modes): max error relative to the largest value.  The audio is
    decoded from the fixture's z: relative RMS error.  The bf16x3 error may be at most 1.1 x the larger of the restatement's own float32 error and
    this library's fp32-mode error (1.1: the margin of DESIGN.md section 2).
    Measured on the MI355X: encoder ref32 9.88e-07, fp32 9.96e-07, bf16x3 9.42e-07; audio ref32 3.94e-07, fp32 6.38e-07,
    bf16x3 5.69e-07."""
    name = "dac_tiny"
    g, cfg, sd = load_golden(name), _cfg(name), _sd(name)
    x = _x(g["pcm"])
    zfix = torch.from_numpy(g["z_nall"])
    ref32 = du.DacRef(cfg, sd)
    ref64 = du.DacRef(cfg, sd)
    ref64.sd = {k: v.double() for k, v in sd.items()}
    d = ref32.cfg["codebook_dim"]
    with torch.no_grad():
        lat64 = ref64.quantize(ref64.encoder(x.cpu().double()), 1)[2]
        aud64 = ref64.decoder(zfix.double())
        lat_r = ref32.quantize(ref32.encoder(x.cpu()), 1)[2]
        aud_r = ref32.decoder(zfix)
    m = _model(name)
    lat_f = m.encode(x, 1)[2].cpu()
    aud_f = m.decode(zfix.cuda()).cpu()
    with _mode(m, "bf16x3"):
        lat_3 = m.encode(x, 1)[2].cpu()
        aud_3 = m.decode(zfix.cuda()).cpu()
    assert lat64.shape[1] == d
    e_enc = {k: _rel(v, lat64) for k, v in (("ref32", lat_r), ("fp32", lat_f), ("bf16x3", lat_3))}
    e_aud = {k: _rel_rms(v, aud64) for k, v in (("ref32", aud_r), ("fp32", aud_f), ("bf16x3", aud_3))}
    print("encoder (stage-0 latents) error against float64:", {k: f"{v:.3g}" for k, v in e_enc.items()})
    print("audio error against float64:", {k: f"{v:.3g}" for k, v in e_aud.items()})
    assert e_enc["bf16x3"] <= 1.1 * max(e_enc["ref32"], e_enc["fp32"]), e_enc
    assert e_aud["bf16x3"] <= 1.1 * max(e_aud["ref32"], e_aud["fp32"]), e_aud


# ---- 7. the invariants of the fp32 path, in bf16x3 -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", ("dac_syn", "dac_tiny"))
def test_bf16x3_batch_independence(name):
    """8 clips against clips 0 / 3 / 7 alone, bitwise.  On dac_tiny the batch of 8 takes 128-row tiles where a single clip takes 64-row tiles."""
    g = load_golden(name)
    xb = _x(_clips("dac-batch", 8, g["pcm"].shape[-1]))
    with _mode(_model(name), "bf16x3") as m:
        zb, cb_, *_ = m.encode(xb)
        ab = m.decode(zb)
        for i in (0, 3, 7):
            z1, c1, *_ = m.encode(xb[i:i + 1])
            assert torch.equal(c1, cb_[i:i + 1]) and torch.equal(z1, zb[i:i + 1]) and torch.equal(m.decode(z1), ab[i:i + 1]), i


@gpu
def test_bf16x3_prefix_property():
    x = _x(load_golden("dac_tiny")["pcm"])
    with _mode(_model("dac_tiny"), "bf16x3") as m:
        full = m.encode(x, 18)[1]
        for n in (1, 2, 6, 12):
            assert torch.equal(m.encode(x, n)[1], full[:, :n])
        assert torch.equal(m.encode(x, 40)[1], full)


@gpu
@pytest.mark.parametrize("name", ("dac_syn", "dac_tiny"))
def test_bf16x3_snake_placement_is_bitwise_neutral(name):
    from esc import _native
    x = _x(load_golden(name)["pcm"])
    m = _model(name)
    default = _native.load().escx_dac_get_snake_maps(m._handle(torch.device("cuda:0"))[1])
    with _mode(m, "bf16x3"):
        z0, c0, l0, cm0, _ = m.encode(x)
        a0 = m.decode(z0)
        try:
            for mask in (0, 1, 2, 4, 8, 16, 31):
                m.set_snake_maps(mask)
                z, c, lat, cm, _ = m.encode(x)
                assert torch.equal(z, z0) and torch.equal(c, c0) and torch.equal(lat, l0) and torch.equal(cm, cm0), mask
                assert torch.equal(m.decode(z0), a0), mask
        finally:
            m.set_snake_maps(default)


def _check_against_restatement(m, x, name):
    out = m(x)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    r = du.DacRef(_cfg(name), sd).forward(x.cpu())
    np.testing.assert_array_equal(out["codes"].cpu().numpy(), r["codes"].numpy())
    assert _rel_rms(out["audio"].cpu(), r["audio"]) < 1e-4
    return out


def _change(m):
    with torch.no_grad():
        m.get_parameter("encoder.block.1.block.0.block.1.weight_g").mul_(1.5)
        m.get_parameter("decoder.model.1.block.0.alpha").add_(0.25)


@gpu
def test_bf16x3_in_place_parameter_change_is_picked_up():
    name = "dac_syn"
    x = _x(load_golden(name)["pcm"])
    m = _fresh(name).set_precision("bf16x3")
    a0 = m(x)["audio"].clone()
    _change(m)
    out = _check_against_restatement(m, x, name)
    assert not torch.equal(out["audio"], a0)


@gpu
def test_bf16x3_after_a_mode_switch_sees_the_current_parameters():
    """The three-term weight image is built in bf16x3, the parameters then change while the handle runs in fp32, and the mode switches back with no
    parameter change in between: the image must be the current parameters', not the one built before."""
    name = "dac_syn"
    x = _x(load_golden(name)["pcm"])
    m = _fresh(name).set_precision("bf16x3")
    a0 = m(x)["audio"].clone()                                      # image of the initial parameters
    m.set_precision("fp32")
    _change(m)
    a1 = m(x)["audio"].clone()                                      # fp32 run re-derives the packed weights
    m.set_precision("bf16x3")
    out = _check_against_restatement(m, x, name)
    assert not torch.equal(out["audio"], a0)
    ref = _fresh(name)
    _change(ref)
    ref.set_precision("bf16x3")
    assert torch.equal(ref(x)["audio"], out["audio"])               # bitwise a model that never held the older image
    assert _rel_rms(out["audio"].cpu(), a1.cpu()) < 1e-4


# ---- 8. every branch of the launcher -------------------------------------------------------------------------------------------------------
@gpu
def test_bf16x3_dispatch_branches_and_the_wide_m_path():
    """Branches of csrc/dac.hip run_layer / csrc/dac_x3.h launch_dac_x3 in bf16x3 and the test that reaches each (Np = rup(Cout, 16)):
      fp32 MFMA, Cin = 1 or Cout = 1 (first encoder layer, tanh layer)      every encode / decode of this file
      64 x 32   (Np <= 32)           dac_syn everywhere; dac_tiny B = 2: encoder width 32, decoder width 18
      64 x 64   (Np <= 64)           dac_tiny B = 2: encoder width 64, decoder width 36 (Np 48)
      64 x 96   (96 pads less)       dac_tiny B = 2: decoder widths 288, 144, 72 (Np 80); dac_base B = 1: 1536 ... 96
      64 x 128  (128 pads less)      dac_tiny B = 2: encoder widths 128, 256, 512; dac_base B = 1
      128 x 32  (>= 512 tiles)       dac_tiny B = 8 (test_bf16x3_batch_independence): encoder width 32, decoder width 18 at 128000 rows
      128 x 64                       here: DAC-Base encoder width 64 at 160000 rows
      128 x 96                       here: DAC-Base decoder widths 192 (80000 rows) and 96 (159920 rows)
      128 x 128                      here: DAC-Base encoder width 128 at 80000 rows
      ConvTranspose1d phase GEMMs, strided and dilated Conv1d, bias / residual epilogues: every model.
    Ten 1 s clips through DAC-Base against the restatement on the device under the near-tie rule; at most 1 % of the rows may be attributed to
    near-ties (the budget of the always-on sweeps), and the fp32 mode must meet the same cap on the same input."""
    name = "dac_base"
    m = _model(name)
    ref = du.DacRef(_cfg(name), {k: v.cuda() for k, v in _sd(name).items()})
    x = _x(_clips("dac-x3-wide", 10, 16000))
    with torch.no_grad():
        ze = ref.encoder(x)
        rz, rc, rl, rcm, rcb, mg = ref.quantize(ze, None, margins=True)
        ra = ref.decoder(rz)
    want, mg = rc.cpu().numpy(), mg.cpu().numpy()
    n_rows = want.shape[0] * want.shape[2]
    for mode in ("fp32", "bf16x3"):
        with _mode(m, mode):
            codes = m.encode(x)[1].cpu().numpy()
            a = m.decode(rz)
        rows = 0
        if not np.array_equal(codes, want):
            rows, bad = du.attribute_codes(ref, ze, None, codes, want, mg)
            assert not bad, (mode, bad[:5])
        print(f"DAC-Base 10 x 1 s {mode}: {rows} of {n_rows} rows attributed to near-ties, audio {_rel_rms(a.cpu(), ra.cpu()):.3g}")
        assert rows <= 0.01 * n_rows, (mode, rows)
        assert _rel_rms(a.cpu(), ra.cpu()) < 1e-4, mode
