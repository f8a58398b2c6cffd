"""The latent gradient of esc.baselines.DAC.decode on the MI355X (include/escx.h escx_dac_decode_tape / escx_dac_decode_backward) against
float64: the REAL reference's fixture (tools/gen_dac_grad_golden.py) and the float64 restatement of tests/dac_util.py that the host test pins
to it.  Accuracy is measured against the reference arithmetic's own float32 error (torch eager on the CPU): err_dev <= 2 * err_eager.

Measured on an MI355X (err_dev / err_eager, fp32 | bf16x3): see DESIGN.md section 13.3."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dac_grad_util as gu
from conftest import load_golden

pytestmark = pytest.mark.gpu
MODES = ("fp32", "bf16x3")
_MODELS = {}


def _model(name):
    from esc.baselines import DAC
    if name not in _MODELS:
        m = DAC(**gu.config(name))
        m.load_state_dict(gu.state_dict(name), strict=True)
        _MODELS[name] = m.cuda().eval()
    return _MODELS[name]


def _fresh(name="dac_syn"):
    from esc.baselines import DAC
    m = DAC(**gu.config(name))
    m.load_state_dict(gu.state_dict(name), strict=True)
    return m.cuda().eval()


@functools.lru_cache(maxsize=None)
def _case(name, B, T):
    """(z, w, d_z float64, err_eager): the fixture's where it has the shape, else seeded inputs and the float64 restatement; computed once."""
    if gu.FIXTURE_CASES.get(name) == (B, T):
        g = load_golden("dac_grad")
        z, w, d64 = g[f"{name}_z"], g[f"{name}_w"], g[f"{name}_d_z"]
    else:
        z, w = gu.inputs(name, B, T)
        d64 = gu.oracle(name, z, w)
    err_eager = gu.rel_l2(gu.oracle(name, z, w, torch.float32), d64)
    for a in (z, w, d64):
        a.setflags(write=False)
    return z, w, d64, err_eager


def _dev(a):
    return torch.from_numpy(np.asarray(a, np.float32)).cuda()


def _grad(m, z, w):
    """(audio, d_z) of sum(decode(z) * w) on the device."""
    zt = _dev(z).requires_grad_(True)
    audio = m.decode(zt)
    assert audio.grad_fn is not None and audio.requires_grad
    (audio * _dev(w)).sum().backward()
    torch.cuda.synchronize()
    return audio.detach(), zt.grad


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,B,T", [("dac_syn", 3, 7), ("dac_syn", 1, 1), ("dac_syn", 2, 96), ("dac_tiny", 2, 5), ("dac_tiny", 1, 1), ("dac_base", 1, 3)])
def test_latent_gradient_against_float64(name, B, T, mode):
    z, w, d64, err_eager = _case(name, B, T)
    m = _model(name)
    m.set_precision(mode)
    try:
        audio, dz = _grad(m, z, w)
        plain = m.decode(_dev(z))
        assert plain.grad_fn is None and torch.equal(audio, plain), "the grad path's audio is not bitwise decode's"
    finally:
        m.set_precision("fp32")
    assert dz.shape == d64.shape and dz.dtype == torch.float32
    err_dev = gu.rel_l2(dz.cpu().numpy(), d64)
    print(f"{name} {B}x{T} {mode}: err_dev {err_dev:.3e}  err_eager {err_eager:.3e}  ratio {err_dev / err_eager:.2f}")
    assert 1e-8 < err_eager < 5e-6, err_eager
    assert err_dev <= 2 * err_eager, (err_dev, err_eager)


@pytest.mark.parametrize("where", ("first", "middle", "last"))
def test_one_sample_cotangent_keeps_the_exact_zeros(where):
    name, B, T = "dac_syn", 2, 96
    z, _, _, _ = _case(name, B, T)
    n = gu.du.output_samples(gu.config(name), T)
    w = np.zeros((B, 1, n))
    w[0, 0, {"first": 0, "middle": n // 2, "last": n - 1}[where]] = 1.0
    d64 = gu.oracle(name, z, w)
    zero = d64 == 0
    assert zero[1].all() and 0 < int(zero[0].sum()) < zero[0].size, "the oracle's support does not exercise the check"
    _, dz = _grad(_model(name), z, w)
    dz = dz.cpu().numpy()
    assert np.array_equal(dz[zero], np.zeros(int(zero.sum()), np.float32)), "nonzero where the float64 oracle is exactly zero"
    assert np.array_equal(dz[1], np.zeros_like(dz[1]))
    assert gu.rel_l2(dz, d64) < 1e-5


def test_zero_cotangent_gives_exactly_zero():
    name, B, T = "dac_syn", 2, 96
    z, w, _, _ = _case(name, B, T)
    _, dz = _grad(_model(name), z, np.zeros_like(w))
    assert np.array_equal(dz.cpu().numpy(), np.zeros(z.shape, np.float32))


@pytest.mark.parametrize("mode", MODES)
def test_batch_independence_and_determinism(mode):
    name, B, T = "dac_syn", 8, 24
    z, w = gu.inputs(name, B, T)
    m = _model(name)
    m.set_precision(mode)
    try:
        _, dz = _grad(m, z, w)
        _, again = _grad(m, z, w)
        assert torch.equal(dz, again), "two backward calls differ"
        for i in (0, 3, 7):
            _, one = _grad(m, z[i:i + 1], w[i:i + 1])
            assert torch.equal(one, dz[i:i + 1]), i
    finally:
        m.set_precision("fp32")


def test_leaf_through_a_linear_map_and_two_graphs_alive():
    name = "dac_syn"
    m = _model(name)
    z1, w1, d1, _ = _case(name, 3, 7)
    z2, w2 = gu.inputs(name, 2, 5)
    _, solo1 = _grad(m, z1, w1)
    _, solo2 = _grad(m, z2, w2)
    # two decode graphs alive at once, backwarded in reverse order of their forwards
    a, b = _dev(z1).requires_grad_(True), _dev(z2).requires_grad_(True)
    out_a, out_b = m.decode(a), m.decode(b)
    (out_b * _dev(w2)).sum().backward()
    (out_a * _dev(w1)).sum().backward()
    assert torch.equal(a.grad, solo1) and torch.equal(b.grad, solo2)
    assert gu.rel_l2(a.grad.cpu().numpy(), d1) < 1e-5 and gu.rel_l2(b.grad.cpu().numpy(), gu.oracle(name, z2, w2)) < 1e-5
    # a leaf feeds a torch linear map, then decode, then a loss: leaf.grad = A^T d_z
    A = gu.seeded("linear", (m.latent_dim, 16), 0.25)
    leaf = _dev(gu.seeded("leaf", (3, 16, 7))).requires_grad_(True)
    zz = torch.einsum("dc,bct->bdt", _dev(A), leaf)
    (m.decode(zz) * _dev(w1)).sum().backward()
    z64 = np.einsum("dc,bct->bdt", A, gu.seeded("leaf", (3, 16, 7)))
    want = np.einsum("dc,bdt->bct", A, gu.oracle(name, z64, w1))
    assert leaf.grad is not None and gu.rel_l2(leaf.grad.cpu().numpy(), want) < 1e-5          # plumbing: 20 x the float32 error of the reference itself


def test_parameters_never_switch_the_path_on_nor_get_a_gradient():
    m = _fresh()
    for p in m.parameters():
        p.requires_grad_(True)
    z, w, _, _ = _case("dac_syn", 3, 7)
    out = m.decode(_dev(z))
    assert out.grad_fn is None and not out.requires_grad
    with torch.no_grad():
        quiet = m.decode(_dev(z).requires_grad_(True))
    assert quiet.grad_fn is None and torch.equal(quiet, out)
    _grad(m, z, w)
    assert all(p.grad is None for p in m.parameters())


def test_device_snake_and_tanh_derivatives_against_fp64():
    """The backward's Snake derivative and 1 - y^2 (escx_dac_test_grad_math) within 2 ulp of fp64 over the grid and under the input-rounding
    rule of test_dac.test_device_snake_and_tanh_against_fp64: alpha * x is rounded once by the formula before the sine (doubling it is exact)."""
    from esc import _native
    lib = _native.load()
    xs = torch.linspace(-20.0, 20.0, 20001, dtype=torch.float32)
    al = torch.linspace(0.1, 3.0, 30, dtype=torch.float32)
    X, A = torch.meshgrid(xs, al, indexing="ij")
    X, A = X.reshape(-1).contiguous(), A.reshape(-1).contiguous()
    xd, ad, out = X.cuda(), A.cuda(), torch.empty(X.numel(), device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    _native.check(lib.escx_dac_test_grad_math(ctypes.c_void_p(xd.data_ptr()), ctypes.c_void_p(ad.data_ptr()), ctypes.c_void_p(out.data_ptr()), X.numel(), 0, st))
    ulp = lambda v: torch.abs(v).clamp_min(2.0 ** -126) * 2.0 ** -23          # noqa: E731
    x64, a64 = X.double(), A.double()
    term = a64 / (a64 + 1e-9) * torch.sin(2.0 * (A * X).double())
    y_r = 1.0 + term
    err = (out.cpu().double() - y_r).abs()
    print(f"snake': max err {float((err / (2 * ulp(y_r) + 2 * ulp(term))).max()):.3f} of the bound")
    assert bool((err <= 2 * ulp(y_r) + 2 * ulp(term)).all()), float((err / ulp(y_r)).max())
    for grid in (X, torch.linspace(-1.0, 1.0, 200001, dtype=torch.float32)):
        yd, o = grid.cuda(), torch.empty(grid.numel(), device="cuda")
        _native.check(lib.escx_dac_test_grad_math(ctypes.c_void_p(yd.data_ptr()), None, ctypes.c_void_p(o.data_ptr()), grid.numel(), 1, st))
        t64 = 1.0 - grid.double() ** 2
        assert bool(((o.cpu().double() - t64).abs() <= 2 * ulp(t64)).all())
    assert lib.escx_dac_test_grad_math(ctypes.c_void_p(xd.data_ptr()), None, ctypes.c_void_p(out.data_ptr()), 4, 0, st) == -1       # mode 0 needs alpha


def test_python_errors_of_the_grad_path():
    z, w, _, _ = _case("dac_syn", 3, 7)
    m = _fresh()
    # padding off: refused on the new path only (the plain path decodes)
    T = next(t for t in range(1, 400) if m._walk(t, m._conv_layers()[2 + 7 * len(m.encoder_rates):]) >= 1)
    m.padding = False
    try:
        zl = torch.zeros(1, m.latent_dim, T, device="cuda")
        assert m.decode(zl).grad_fn is None
        with pytest.raises(NotImplementedError):
            m.decode(zl.clone().requires_grad_(True))
    finally:
        m.padding = True
    # an in-place parameter edit between forward and backward
    zt = _dev(z).requires_grad_(True)
    out = m.decode(zt)
    with torch.no_grad():
        m.get_parameter("decoder.model.1.block.0.alpha").add_(0.25)
    with pytest.raises(RuntimeError, match="changed in place"):
        (out * _dev(w)).sum().backward()
    assert zt.grad is None
    # double backward
    zt = _dev(z).requires_grad_(True)
    (g,) = torch.autograd.grad((m.decode(zt) * _dev(w)).sum(), zt, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    # training mode refuses before anything else
    m.train()
    with pytest.raises(NotImplementedError):
        m.decode(_dev(z).requires_grad_(True))
    m.eval()


def test_c_level_errors_leave_the_handle_usable():
    from esc import _native
    z, w, _, _ = _case("dac_syn", 3, 7)
    m = _fresh()
    zc, wc = _dev(z), _dev(w).contiguous()
    before = m.decode(zc)
    _, want = _grad(m, z, w)
    lib, hd, flat, dev, st = m._ctx(zc, "z")
    B, D, T = zc.shape
    P = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    v = m._version()
    floats = lib.escx_dac_decode_tape_floats(hd, B, T)
    assert floats > 64 and floats % 64 == 0
    assert lib.escx_dac_decode_tape_floats(hd, B, 0) == 0
    tape, audio, dz = torch.empty(floats, device="cuda"), torch.empty_like(before), torch.full((B, D, T), 7.0, device="cuda")
    assert lib.escx_dac_decode_tape(hd, P(flat), v, P(zc), B, T, P(audio), P(tape), floats - 64, st) == -1                 # a tape of the wrong size
    _native.check(lib.escx_dac_decode_tape(hd, P(flat), v, P(zc), B, T, P(audio), P(tape), floats, st))
    assert torch.equal(audio, before)
    rc = lib.escx_dac_decode_backward(hd, P(flat), v + 1, P(tape), floats, P(wc), B, T, P(dz), st)                      # a stale parameter version
    assert rc in (-4, -1) and b"version" in lib.escx_last_error()
    assert lib.escx_dac_decode_backward(hd, P(flat), v, P(torch.zeros(floats, device="cuda")), floats, P(wc), B, T, P(dz), st) == -1     # not a tape
    torch.cuda.synchronize()
    assert bool((dz == 7.0).all()), "a refused backward wrote its output"
    _native.check(lib.escx_dac_set_padding(hd, 0))
    try:
        assert lib.escx_dac_decode_tape_floats(hd, B, T) == -2
        assert lib.escx_dac_decode_tape(hd, P(flat), v, P(zc), B, T, P(audio), P(tape), floats, st) == -2
        assert lib.escx_dac_decode_backward(hd, P(flat), v, P(tape), floats, P(wc), B, T, P(dz), st) == -2
    finally:
        _native.check(lib.escx_dac_set_padding(hd, 1))
    assert torch.equal(m.decode(zc), before), "the handle decodes differently after the refused calls"
    _native.check(lib.escx_dac_decode_backward(hd, P(flat), v, P(tape), floats, P(wc), B, T, P(dz), st))
    torch.cuda.synchronize()
    assert torch.equal(dz, want)
