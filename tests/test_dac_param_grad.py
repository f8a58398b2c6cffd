"""The decoder parameter gradients of esc.baselines.DAC.decode after set_trainable("decoder") on the MI355X (include/escx.h
escx_dac_decode_backward_params) against float64: the REAL reference's fixture (tools/gen_dac_param_grad_golden.py) where it stores a tensor, else
the float64 restatement of tests/dac_util.py that the host test pins to it.  Accuracy is measured per kind of parameter (bias, weight_g, weight_v,
alpha) against the reference arithmetic's own float32 error (torch eager on the CPU), tests/dac_param_grad_util.check_rule:
rms(err_dev) <= 2 rms(err_eager) and every tensor's err_dev <= 2 max(err_eager) of its kind.

Measured on an MI355X (err_dev / err_eager per kind and shape): see DESIGN.md section 13.5."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dac_grad_util as gu
import dac_param_grad_util as pu
from conftest import load_golden

pytestmark = pytest.mark.gpu
MODES = ("fp32", "bf16x3")
_MODELS = {}


def _fresh(name="dac_syn", sd=None):
    from esc.baselines import DAC
    m = DAC(**gu.config(name))
    m.load_state_dict(gu.state_dict(name) if sd is None else sd, strict=True)
    return m.cuda().eval()


def _model(name):
    """One model per configuration, switched to the decoder; a test that changes its switches puts them back."""
    if name not in _MODELS:
        _MODELS[name] = _fresh(name).set_trainable("decoder")
    return _MODELS[name]


@functools.lru_cache(maxsize=None)
def _case(name, B, T):
    """(z, w, g64 {key: float64 gradient}, err_eager {key: error of float32 eager}): g64 is the fixture's tensor where it stores one in full,
    else the float64 restatement's; computed once."""
    z, w = gu.inputs(name, B, T)
    g64 = pu.oracle(name, z, w)
    if pu.FIXTURE_CASES.get(name) == (B, T):
        g = load_golden("dac_param_grad")
        assert np.array_equal(g[f"{name}_z"], z) and np.array_equal(g[f"{name}_w"], w)
        for k in g64:
            if f"{name}_g/{k}" in g.files:
                g64[k] = g[f"{name}_g/{k}"]
    err_eager = pu.errors(pu.oracle(name, z, w, torch.float32), g64)
    for a in (z, w, *g64.values()):
        a.setflags(write=False)
    return z, w, g64, err_eager


def _dev(a):
    return torch.from_numpy(np.asarray(a, np.float32)).cuda()


def _decoder_named(m):
    return {k: p for k, p in m.named_parameters() if k.startswith("decoder.")}


def _run(m, z, w, z_grad=True, want=None, keep=False):
    """(audio, z.grad, {key: p.grad}) of sum(decode(z) * w) on the device with the decoder parameters in `want` (all by default) requiring gradients."""
    named = _decoder_named(m)
    for k, p in m.named_parameters():
        p.requires_grad_(k in named and (want is None or k in want))
        if not keep:
            p.grad = None
    zt = _dev(z).requires_grad_(z_grad)
    audio = m.decode(zt)
    assert audio.grad_fn is not None and audio.requires_grad
    (audio * _dev(w)).sum().backward()
    torch.cuda.synchronize()
    return audio.detach(), zt.grad, {k: p.grad for k, p in m.named_parameters() if p.grad is not None}


def _np(grads):
    return {k: v.detach().cpu().numpy() for k, v in grads.items()}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,B,T", [("dac_syn", 3, 7), ("dac_tiny", 2, 5), ("dac_tiny", 1, 1), ("dac_syn", 3, 37), ("dac_base", 1, 3)])
def test_parameter_gradients_against_float64(name, B, T, mode):
    z, w, g64, err_eager = _case(name, B, T)
    m = _model(name)
    m.set_precision(mode)
    try:
        audio, dz, grads = _run(m, z, w)
        with torch.no_grad():
            plain = m.decode(_dev(z))
        assert torch.equal(audio, plain), "the parameter path's audio is not bitwise decode's"
    finally:
        m.set_precision("fp32")
    assert list(grads) == list(g64), "not exactly the decoder's parameters got a gradient"
    named = _decoder_named(m)
    for k, g in grads.items():
        assert g.shape == named[k].shape == g64[k].shape and g.dtype == torch.float32, k
    assert dz is not None and dz.shape == z.shape
    pu.check_rule(pu.errors(_np(grads), g64), err_eager, f"{name} {B}x{T} {mode}")


def test_more_than_one_slice_and_a_ragged_last_slice():
    """dac_syn at 3 x 37: the contractions run over 111, 222 and 444 rows - no multiple of the 32-row chunk or of the 128-row slice - and every
    layer from the first block's residual units on runs 2 or 4 slices (the accuracy at this shape is test_parameter_gradients_against_float64's)."""
    m = _model("dac_syn")
    lib, hd, _, _, _ = m._ctx(torch.zeros(1, device="cuda"), "z")
    n_layers = 2 + 7 * len(m.decoder_rates)
    slices = [lib.escx_dac_param_grad_slices(hd, 3, 37, i) for i in range(n_layers)]
    print("slices per decoder layer at 3 x 37:", slices)
    assert slices[0] == 1 and slices[1] == 1 and sum(s > 1 for s in slices) >= 2 and max(slices) == 4
    assert all(s == 2 for s in slices[2:9]) and all(s == 4 for s in slices[9:])
    assert lib.escx_dac_param_grad_slices(hd, 3, 37, n_layers) == 0 and lib.escx_dac_param_grad_slices(hd, 3, 0, 0) == 0
    assert lib.escx_dac_param_grad_workspace_floats(hd) > 0


@pytest.mark.parametrize("mode", MODES)
def test_bitwise_audio_latent_gradient_determinism_and_accumulation(mode):
    name, B, T = "dac_syn", 3, 37
    z, w = gu.inputs(name, B, T)
    m = _model(name)
    m.set_precision(mode)
    try:
        audio, dz, g1 = _run(m, z, w)
        g1 = {k: v.clone() for k, v in g1.items()}
        _, dz2, g2 = _run(m, z, w)
        assert torch.equal(dz, dz2) and list(g1) == list(g2) and all(torch.equal(g1[k], g2[k]) for k in g1), "two backward calls differ"
        _, _, acc = _run(m, z, w, keep=True)                    # p.grad still holds the run before: autograd adds
        assert all(torch.equal(acc[k], 2 * g1[k]) for k in g1), "two accumulated backwards are not twice one"
        # the frozen decoder falls back to the latent-only path: the same audio and the same d_z, bit for bit
        for p in m.parameters():
            p.requires_grad_(False)
            p.grad = None
        zt = _dev(z).requires_grad_(True)
        frozen = m.decode(zt)
        assert type(frozen.grad_fn).__name__.startswith("_DecodeGrad")
        (frozen * _dev(w)).sum().backward()
        assert torch.equal(frozen.detach(), audio) and torch.equal(zt.grad, dz), "d_z differs from the latent-only backward's"
        assert all(p.grad is None for p in m.parameters())
        with torch.no_grad():
            assert torch.equal(m.decode(_dev(z)), audio)
    finally:
        m.set_precision("fp32")


def test_selective_gradients():
    name, B, T = "dac_syn", 3, 7
    z, w, g64, _ = _case(name, B, T)
    m = _model(name)
    _, dz, full = _run(m, z, w)
    full = {k: v.clone() for k, v in full.items()}
    alphas = [k for k in g64 if pu.kind(k) == "alpha"]
    one_v = ["decoder.model.1.block.2.block.1.weight_v"]
    assert one_v[0] in g64
    for want in (alphas, one_v):
        _, dz_s, got = _run(m, z, w, z_grad=False, want=want)
        assert dz_s is None and list(got) == want, "not exactly the selected parameters got a gradient"
        assert all(torch.equal(got[k], full[k]) for k in want)
        assert all(p.grad is None for k, p in m.named_parameters() if k not in want)
    # forward(x) goes through decode: the decoder's parameters get gradients, the frozen encoder and quantiser none
    for k, p in m.named_parameters():
        p.requires_grad_(True)
        p.grad = None
    x = _dev(gu.seeded("x:forward", (2, 1, 64), 0.5))
    m(x)["audio"].sum().backward()
    assert all((p.grad is not None) == k.startswith("decoder.") for k, p in m.named_parameters())
    # the switch set back: today's behaviour, no p.grad whatever requires_grad says
    m.set_trainable(None)
    try:
        for p in m.parameters():
            p.grad = None
        zt = _dev(z).requires_grad_(True)
        out = m.decode(zt)
        assert type(out.grad_fn).__name__.startswith("_DecodeGrad")
        (out * _dev(w)).sum().backward()
        assert torch.equal(zt.grad, dz) and all(p.grad is None for p in m.parameters())
        assert m.decode(_dev(z)).grad_fn is None
    finally:
        m.set_trainable("decoder")


def test_three_optimiser_steps():
    name, B, T = "dac_syn", 3, 7
    z, _ = gu.inputs(name, B, T)
    m = _fresh(name).set_trainable("decoder")
    for k, p in m.named_parameters():
        p.requires_grad_(k.startswith("decoder."))
    target = gu.seeded("target", (B, 1, gu.du.output_samples(gu.config(name), T)), 0.5)
    opt = torch.optim.SGD(list(m.decoder_parameters()), lr=0.05)
    zd, td = _dev(z), _dev(target)
    losses = []
    for step in range(3):
        sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        opt.zero_grad(set_to_none=True)
        loss = (m.decode(zd) - td).pow(2).mean()
        loss.backward()
        losses.append(loss.item())
        if step == 1:                                           # the gradients after one step: the re-pack and the refreshed transposed images
            g64 = pu.oracle(name, z, target, sd=sd, mse=True)
            err_eager = pu.errors(pu.oracle(name, z, target, torch.float32, sd=sd, mse=True), g64)
            got = _np({k: p.grad for k, p in m.named_parameters() if p.grad is not None})
            assert list(got) == list(g64)
            pu.check_rule(pu.errors(got, g64), err_eager, f"{name} {B}x{T} after one SGD step")
        before = {k: p.detach().clone() for k, p in _decoder_named(m).items()}
        opt.step()
        assert all(not torch.equal(before[k], p) for k, p in _decoder_named(m).items()), "a decoder parameter did not move"
        with torch.no_grad():
            stepped = m.decode(zd)
        twin = _fresh(name, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
        assert torch.equal(stepped, twin.decode(zd)), f"step {step}: the stepped model decodes differently from a fresh model with its state_dict"
    print("losses:", losses)
    assert losses[2] < losses[0]


def test_python_errors_of_the_parameter_path():
    z, w, _, _ = _case("dac_syn", 3, 7)
    m = _fresh().set_trainable("decoder")
    # padding off: refused on the new path only (the plain path decodes)
    T = next(t for t in range(1, 400) if m._walk(t, m._conv_layers()[2 + 7 * len(m.encoder_rates):]) >= 1)
    m.padding = False
    try:
        zl = torch.zeros(1, m.latent_dim, T, device="cuda")
        with torch.no_grad():
            assert m.decode(zl).grad_fn is None
        with pytest.raises(NotImplementedError):
            m.decode(zl)
    finally:
        m.padding = True
    # an in-place parameter edit between forward and backward
    out = m.decode(_dev(z))
    with torch.no_grad():
        m.get_parameter("decoder.model.1.block.0.alpha").add_(0.25)
    with pytest.raises(RuntimeError, match="changed in place"):
        (out * _dev(w)).sum().backward()
    assert all(p.grad is None for p in m.parameters())
    # double backward
    p0 = m.get_parameter("decoder.model.0.bias")
    (g,) = torch.autograd.grad((m.decode(_dev(z)) * _dev(w)).sum(), p0, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    # training mode refuses before anything else
    m.train()
    with pytest.raises(NotImplementedError):
        m.decode(_dev(z))
    m.eval()


def test_c_level_errors_leave_the_handle_and_the_other_slots_alone():
    from esc import _native
    z, w, _, _ = _case("dac_syn", 3, 7)
    m = _fresh().set_trainable("decoder")
    zc, wc = _dev(z), _dev(w).contiguous()
    with torch.no_grad():
        before = m.decode(zc)
    _, want_dz, want = _run(m, z, w)
    lib, hd, flat, dev, st = m._ctx(zc, "z")
    B, D, T = zc.shape
    P = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    v = m._version()
    floats = lib.escx_dac_decode_tape_floats(hd, B, T)
    tape, audio = torch.empty(floats, device="cuda"), torch.empty_like(before)
    _native.check(lib.escx_dac_decode_tape(hd, P(flat), v, P(zc), B, T, P(audio), P(tape), floats, st))
    layout = m._flat[dev.index if dev.index is not None else torch.cuda.current_device()]["layout"]
    first = min(off for k, off, n in layout if k.startswith("decoder."))
    assert all(off >= first for k, off, n in layout if k.startswith("decoder.")) and first > 0 and layout[-1][1] + layout[-1][2] == flat.numel()
    grad, dz = torch.full_like(flat, 7.0), torch.full((B, D, T), 7.0, device="cuda")
    call = lambda ver, tp, zz, gg: lib.escx_dac_decode_backward_params(hd, P(flat), ver, P(tp), floats, zz, P(wc), B, T, P(dz), gg, st)      # noqa: E731
    rc = call(v + 1, tape, P(zc), P(grad))                                                                      # a stale parameter version
    assert rc == -4 and b"version" in lib.escx_last_error() and str(v).encode() in lib.escx_last_error() and str(v + 1).encode() in lib.escx_last_error()
    assert call(v, torch.zeros(floats, device="cuda"), P(zc), P(grad)) == -1                                    # not a tape
    assert lib.escx_dac_decode_backward_params(hd, P(flat), v, P(tape), floats - 64, P(zc), P(wc), B, T, P(dz), P(grad), st) == -1      # the wrong size
    assert call(v, tape, P(zc), None) == -1 and call(v, tape, None, P(grad)) == -1                              # NULL grad_flat, NULL z
    _native.check(lib.escx_dac_set_padding(hd, 0))
    try:
        assert call(v, tape, P(zc), P(grad)) == -2
    finally:
        _native.check(lib.escx_dac_set_padding(hd, 1))
    torch.cuda.synchronize()
    assert bool((grad == 7.0).all()) and bool((dz == 7.0).all()), "a refused backward wrote an output"
    with torch.no_grad():
        assert torch.equal(m.decode(zc), before), "the handle decodes differently after the refused calls"
    assert call(v, tape, P(zc), P(grad)) == 0
    torch.cuda.synchronize()
    assert bool((grad[:first] == 7.0).all()), "a float outside the decoder's slots was written"
    assert torch.equal(dz, want_dz)
    for k, off, n in layout:
        if k.startswith("decoder."):
            assert torch.equal(grad[off:off + n], want[k].reshape(-1)), k
    # without d_z the parameter gradients are the same
    grad2 = torch.full_like(flat, 7.0)
    assert lib.escx_dac_decode_backward_params(hd, P(flat), v, P(tape), floats, P(zc), P(wc), B, T, None, P(grad2), st) == 0
    torch.cuda.synchronize()
    assert torch.equal(grad2, grad)
