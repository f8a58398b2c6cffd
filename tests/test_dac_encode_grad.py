"""The audio gradient of esc.baselines.DAC.encode / forward on the MI355X (include/escx.h escx_dac_encode_tape / escx_dac_encode_backward)
against float64: the REAL reference's fixture (tools/gen_dac_encode_grad_golden.py) and the float64 restatement of
tests/dac_encode_grad_util.py that the host test pins to it.  Both oracles run with the device's codes forced (the commitment term depends on the
chosen code).  Accuracy is measured against the reference arithmetic's own float32 error (torch eager on the CPU): err_dev <= 2 * err_eager.

Measured on an MI355X (err_dev / err_eager, fp32 | bf16x3): see DESIGN.md section 13.4."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import dac_encode_grad_util as eu
from conftest import load_golden

pytestmark = pytest.mark.gpu
MODES = ("fp32", "bf16x3")
_MODELS = {}


def _model(name):
    from esc.baselines import DAC
    if name not in _MODELS:
        m = DAC(**eu.config(name))
        m.load_state_dict(eu.state_dict(name), strict=True)
        _MODELS[name] = m.cuda().eval()
    return _MODELS[name]


def _fresh(name="dac_syn"):
    from esc.baselines import DAC
    m = DAC(**eu.config(name))
    m.load_state_dict(eu.state_dict(name), strict=True)
    return m.cuda().eval()


def _dev(a):
    return torch.from_numpy(np.asarray(a, np.float32)).cuda()


def _loss(out, cot):
    z, _, lat, cm, _ = out
    terms = {"z": z, "latents": lat, "cm": cm}
    return sum((terms[k] * _dev(w)).sum() for k, w in cot.items())


def _grad(m, x, cot, n=None):
    """(encode's outputs detached, d_x) of sum_k sum(out_k * cot_k) on the device."""
    xt = _dev(x).requires_grad_(True)
    out = m.encode(xt, n)
    z, codes, lat, cm, cb = out
    assert z.grad_fn is not None and lat.grad_fn is not None and cm.grad_fn is not None
    assert not codes.requires_grad and not cb.requires_grad
    _loss(out, cot).backward()
    torch.cuda.synchronize()
    return tuple(o.detach() for o in out), xt.grad


def _same_values(got, plain):
    for a, b in zip(got, plain):
        assert b.grad_fn is None and not b.requires_grad
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), "the grad path's values are not bitwise encode's"


@functools.lru_cache(maxsize=None)
def _oracles(name, B, L, n, codes_key, counts=None, whole=False):
    """(d_x float64, err_eager) with the given codes forced: the fixture's d_x where it has the case and the same codes, else the float64
    restatement; the float32 side is torch eager of the restatement on this machine's CPU.  Computed once per case."""
    codes = np.frombuffer(codes_key, np.int64).reshape(B, -1, eu.shapes(name, B, L, n)[1])
    x, cot = eu.inputs(name, B, L, n)
    if whole:
        cot = {"audio": eu.seeded(f"w_audio:{name}:{B}x{L}", (B, 1, L))}
    d64 = None
    if eu.FIXTURE_CASES.get(name) == (B, L, n) and counts is None and not whole:
        g = load_golden("dac_encode_grad")
        if np.array_equal(g[f"{name}_codes"].astype(np.int64), codes):
            d64 = g[f"{name}_d_x"]
    kw = dict(codes=codes, counts=None if counts is None else list(counts), whole=whole)
    if d64 is None:
        d64 = eu.oracle(name, x, cot, n, **kw)
    err_eager = eu.rel_l2(eu.oracle(name, x, cot, n, torch.float32, **kw), d64)
    d64.setflags(write=False)
    return d64, err_eager


def _rule(tag, dx, d64, err_eager):
    assert dx.shape == d64.shape and dx.dtype == torch.float32
    err_dev = eu.rel_l2(dx.cpu().numpy(), d64)
    print(f"{tag}: err_dev {err_dev:.3e}  err_eager {err_eager:.3e}  ratio {err_dev / err_eager:.2f}")
    assert 1e-8 < err_eager < 5e-6, err_eager
    assert err_dev <= 2 * err_eager, (err_dev, err_eager)


CASES = [("dac_syn", 3, 28, 4), ("dac_syn", 1, 4, 4), ("dac_syn", 2, 1027, 3), ("dac_tiny", 2, 1600, 18), ("dac_tiny", 1, 335, 5), ("dac_base", 1, 960, 18)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,B,L,n", CASES)
def test_audio_gradient_against_float64(name, B, L, n, mode):
    x, cot = eu.inputs(name, B, L, n)
    m = _model(name)
    m.set_precision(mode)
    try:
        got, dx = _grad(m, x, cot, n)
        _same_values(got, m.encode(_dev(x), n))
    finally:
        m.set_precision("fp32")
    d64, err_eager = _oracles(name, B, L, n, got[1].cpu().numpy().tobytes())
    _rule(f"{name} {B}x{L} n{n} {mode}", dx, d64, err_eager)


@pytest.mark.parametrize("t", (0, 128, 255))
def test_one_frame_cotangent_keeps_the_exact_zeros(t):
    name, B, L, n = "dac_syn", 2, 1027, 3
    x, _ = eu.inputs(name, B, L, n)
    D, T, n, d = eu.shapes(name, B, L, n)
    assert T == 256
    w = np.zeros((B, D, T))
    w[0, :, t] = 1.0
    m = _model(name)
    got, dx = _grad(m, x, {"z": w}, n)
    d64 = eu.oracle(name, x, {"z": w}, n, codes=got[1].cpu().numpy())
    zero = d64 == 0
    assert zero[1].all() and 0 < int(zero[0].sum()) < zero[0].size, "the oracle's support does not exercise the check"
    dx = dx.cpu().numpy()
    assert np.array_equal(dx[zero], np.zeros(int(zero.sum()), np.float32)), "nonzero where the float64 oracle is exactly zero"
    assert np.array_equal(dx[1], np.zeros_like(dx[1]))
    assert eu.rel_l2(dx, d64) < 1e-5


def test_zero_cotangent_gives_exactly_zero():
    name, B, L, n = "dac_syn", 2, 1027, 3
    x, cot = eu.inputs(name, B, L, n)
    _, dx = _grad(_model(name), x, {k: np.zeros_like(w) for k, w in cot.items()}, n)
    assert np.array_equal(dx.cpu().numpy(), np.zeros(x.shape, np.float32))


def test_uncovered_rows_of_a_strided_convolution_are_zero_not_stale_scratch():
    """dac_tiny at 335 samples: the second block's stride-4 convolution sees 167 rows and its last row lies under no output tap.  The handle's
    scratch is first filled by a larger backward; the small one must not show it."""
    m = _model("dac_tiny")
    xb, cb = eu.inputs("dac_tiny", 2, 1600, 18)
    _grad(m, xb, cb, 18)
    name, B, L, n = "dac_tiny", 1, 335, 5
    x, cot = eu.inputs(name, B, L, n)
    got, dx = _grad(m, x, cot, n)
    clean, dx2 = _grad(_fresh(name), x, cot, n)
    assert torch.equal(dx, dx2), "the gradient depends on what the scratch held"
    assert eu.rel_l2(dx.cpu().numpy(), eu.oracle(name, x, cot, n, codes=got[1].cpu().numpy())) < 1e-5


@pytest.mark.parametrize("mode", MODES)
def test_batch_independence_and_determinism(mode):
    name, B, L, n = "dac_syn", 8, 96, 4
    x, cot = eu.inputs(name, B, L, n)
    cot = {k: cot[k] for k in ("z", "latents")}          # the commitment mean carries 1 / B of the call
    m = _model(name)
    m.set_precision(mode)
    try:
        _, dx = _grad(m, x, cot, n)
        _, again = _grad(m, x, cot, n)
        assert torch.equal(dx, again), "two backward calls differ"
        for i in (0, 3, 7):
            _, one = _grad(m, x[i:i + 1], {k: w[i:i + 1] for k, w in cot.items()}, n)
            assert torch.equal(one, dx[i:i + 1]), i
    finally:
        m.set_precision("fp32")


def test_per_clip_counts():
    name, B, L, n = "dac_syn", 3, 28, 4
    counts = [1, 4, 2]
    x, cot = eu.inputs(name, B, L, n)
    D, T, n, d = eu.shapes(name, B, L, n)
    m = _model(name)
    got, dx = _grad(m, x, cot, counts)
    _same_values(got, m.encode(_dev(x), counts))
    assert got[1].shape == (B, 4, T) and bool((got[1][0, 1:] == -1).all())
    zl = {k: cot[k] for k in ("z", "latents")}
    _, dzl = _grad(m, x, zl, counts)
    for b, nb in enumerate(counts):
        _, one = _grad(m, x[b:b + 1], {"z": cot["z"][b:b + 1], "latents": cot["latents"][b:b + 1, :nb * d]}, nb)
        assert torch.equal(one, dzl[b:b + 1]), b
    d64, err_eager = _oracles(name, B, L, n, got[1].cpu().numpy().tobytes(), counts=tuple(counts))
    _rule(f"{name} {B}x{L} per-clip {counts}", dx, d64, err_eager)
    # a tensor of counts takes the same path
    xt = _dev(x).requires_grad_(True)
    out = m.encode(xt, torch.tensor(counts))
    _loss(out, cot).backward()
    assert torch.equal(xt.grad, dx)


def test_forward_end_to_end():
    name, B, L = "dac_syn", 2, 30                         # not a multiple of the hop: the pad and the trim are in the graph
    m = _model(name)
    x = eu.seeded(f"x:{name}:{B}x{L}:fwd", (B, 1, L), 0.5)
    w = eu.seeded(f"w_audio:{name}:{B}x{L}", (B, 1, L))
    plain = m(_dev(x))
    xt = _dev(x).requires_grad_(True)
    out = m(xt)
    for k, v in plain.items():
        assert v.grad_fn is None and torch.equal(out[k].detach(), v), k
    assert out["audio"].shape == (B, 1, L)
    (out["audio"] * _dev(w)).sum().backward()
    codes = out["codes"].cpu().numpy()
    ref = eu.DacRefE(eu.config(name), eu.state_dict(name), torch.float64)
    d64 = eu.grad_of(lambda t: ref.forward_dict(t, None, torch.from_numpy(codes)), x, {"audio": w}, torch.float64)
    ref32 = eu.DacRefE(eu.config(name), eu.state_dict(name), torch.float32)
    d32 = eu.grad_of(lambda t: ref32.forward_dict(t, None, torch.from_numpy(codes)), x, {"audio": w}, torch.float32)
    _rule(f"{name} forward {B}x{L}", xt.grad, d64, eu.rel_l2(d32, d64))
    # every differentiable output reaches x.grad
    for k in ("audio", "z", "latents", "vq/commitment_loss"):
        xk = _dev(x).requires_grad_(True)
        o = m(xk)[k]
        assert o.grad_fn is not None, k
        o.sum().backward()
        assert xk.grad is not None and float(xk.grad.abs().sum()) > 0, k
    o = m(_dev(x).requires_grad_(True))
    assert not o["codes"].requires_grad and not o["vq/codebook_loss"].requires_grad


def test_leaf_through_a_linear_map_and_two_graphs_alive():
    name = "dac_syn"
    m = _model(name)
    x1, c1 = eu.inputs(name, 3, 28, 4)
    x2, c2 = eu.inputs(name, 2, 1027, 3)
    g1, solo1 = _grad(m, x1, c1, 4)
    g2, solo2 = _grad(m, x2, c2, 3)
    # two encode graphs alive at once, backwarded in reverse order of their forwards
    a, b = _dev(x1).requires_grad_(True), _dev(x2).requires_grad_(True)
    out_a, out_b = m.encode(a, 4), m.encode(b, 3)
    _loss(out_b, c2).backward()
    _loss(out_a, c1).backward()
    assert torch.equal(a.grad, solo1) and torch.equal(b.grad, solo2)
    # a leaf feeds a torch linear map over time, then encode, then a loss: leaf.grad = A^T d_x
    A = eu.seeded("linear", (28, 12), 0.25)
    leaf0 = eu.seeded("leaf", (3, 1, 12))
    leaf = _dev(leaf0).requires_grad_(True)
    out = m.encode(torch.einsum("lc,bic->bil", _dev(A), leaf), 4)
    _loss(out, c1).backward()
    x64 = np.einsum("lc,bic->bil", A, leaf0)
    want = np.einsum("lc,bil->bic", A, eu.oracle(name, x64, c1, 4, codes=out[1].cpu().numpy()))
    assert leaf.grad is not None and eu.rel_l2(leaf.grad.cpu().numpy(), want) < 1e-5          # plumbing: 20 x the float32 error of the reference itself


def test_path_selection():
    m = _fresh()
    for p in m.parameters():
        p.requires_grad_(True)
    x, cot = eu.inputs("dac_syn", 3, 28, 4)
    out = m.encode(_dev(x), 4)
    assert all(o.grad_fn is None and not o.requires_grad for o in out)
    with torch.no_grad():
        quiet = m.encode(_dev(x).requires_grad_(True), 4)
    _same_values(quiet, out)
    zs, codes, lat = m.encode_sweep(_dev(x).requires_grad_(True), [2, 4])
    assert zs.grad_fn is None and lat.grad_fn is None and torch.equal(zs[1], out[0]) and torch.equal(codes, out[1])
    f = m(_dev(x))
    assert all(v.grad_fn is None for v in f.values())
    got, _ = _grad(m, x, cot, 4)
    _same_values(got, out)
    assert all(p.grad is None for p in m.parameters())


def test_python_errors_of_the_grad_path():
    x, cot = eu.inputs("dac_syn", 3, 28, 4)
    m = _fresh()
    # padding off: refused on the new path only (the plain path encodes)
    L = next(l for l in range(1, 4000) if m._walk(l, m._conv_layers()[:2 + 7 * len(m.encoder_rates)]) >= 1)
    m.padding = False
    try:
        xl = torch.zeros(1, 1, L, device="cuda")
        assert m.encode(xl)[0].grad_fn is None
        with pytest.raises(NotImplementedError):
            m.encode(xl.clone().requires_grad_(True))
    finally:
        m.padding = True
    # an in-place parameter edit between forward and backward
    xt = _dev(x).requires_grad_(True)
    out = m.encode(xt, 4)
    with torch.no_grad():
        m.get_parameter("encoder.block.1.block.0.block.0.alpha").add_(0.25)
    with pytest.raises(RuntimeError, match="changed in place"):
        _loss(out, cot).backward()
    assert xt.grad is None
    # double backward
    xt = _dev(x).requires_grad_(True)
    (g,) = torch.autograd.grad(_loss(m.encode(xt, 4), cot), xt, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    # training mode refuses before anything else
    m.train()
    with pytest.raises(NotImplementedError):
        m.encode(_dev(x).requires_grad_(True))
    with pytest.raises(NotImplementedError):
        m(_dev(x).requires_grad_(True))
    m.eval()


def test_c_level_errors_leave_the_handle_usable():
    from esc import _native
    x, cot = eu.inputs("dac_syn", 3, 28, 4)
    m = _fresh()
    xc = _dev(x).contiguous()
    before = m.encode(xc, 4)
    _, want = _grad(m, x, cot, 4)
    lib, hd, flat, dev, st = m._ctx(xc, "audio_data")
    B, _, L = xc.shape
    D, T, n, d = eu.shapes("dac_syn", B, L, 4)
    P = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    v = m._version()
    floats = lib.escx_dac_encode_tape_floats(hd, B, L, n)
    assert floats > 64 and floats % 64 == 0
    assert lib.escx_dac_encode_tape_floats(hd, B, 0, n) == 0 and lib.escx_dac_encode_tape_floats(hd, B, L, 0) == 0
    assert lib.escx_dac_encode_tape_floats(hd, B, L, 99) == floats and lib.escx_dac_encode_tape_floats(hd, B, L, 2) < floats
    z, codes, lat, losses = torch.empty_like(before[0]), torch.empty_like(before[1]), torch.empty_like(before[2]), torch.empty(2, device="cuda")
    tape, dx = torch.empty(floats, device="cuda"), torch.full((B, 1, L), 7.0, device="cuda")
    wz, wl, wc = _dev(cot["z"]).contiguous(), _dev(cot["latents"]).contiguous(), _dev(cot["cm"])

    def fwd(tp, nfl):
        return lib.escx_dac_encode_tape(hd, P(flat), v, P(xc), B, L, n, None, P(z), P(codes), P(lat), P(losses), P(tp), nfl, st)

    def bwd(ver, tp, nfl):
        return lib.escx_dac_encode_backward(hd, P(flat), ver, P(tp), nfl, P(wz), P(wl), P(wc), B, L, P(dx), st)

    dzz = torch.full((B, D, T), 7.0, device="cuda")

    def refused(rc, want_rc):
        """one refused call: its status, no output written, and the handle encodes bitwise as before"""
        assert rc == want_rc, (rc, lib.escx_last_error())
        _same_values(m.encode(xc, 4), before)
        assert bool((dx == 7.0).all()) and bool((dzz == 7.0).all()), "a refused backward wrote its output"

    refused(fwd(tape, floats - 64), -1)                                                              # a tape of the wrong size
    _native.check(fwd(tape, floats))
    assert torch.equal(z, before[0]) and torch.equal(codes, before[1]) and torch.equal(lat, before[2])
    assert torch.equal(losses[0], before[3]) and torch.equal(losses[1], before[4])
    rc = bwd(v + 1, tape, floats)                                                                    # a stale parameter version
    msg = lib.escx_last_error()
    assert b"version" in msg and str(v).encode() in msg and str(v + 1).encode() in msg
    refused(rc, -4)
    refused(bwd(v, torch.zeros(floats, device="cuda"), floats), -1)                                  # not a tape
    refused(bwd(v, tape[:floats - 64], floats - 64), -1)                                             # the wrong size
    # a decode tape handed to the encode backward, and the reverse
    zd = before[0].contiguous()
    dfl = lib.escx_dac_decode_tape_floats(hd, B, T)
    dtape, audio = torch.empty(max(dfl, floats), device="cuda"), torch.empty(B, 1, m.output_samples(T), device="cuda")
    _native.check(lib.escx_dac_decode_tape(hd, P(flat), v, P(zd), B, T, P(audio), P(dtape), dfl, st))
    refused(bwd(v, dtape, dfl), -1)
    refused(lib.escx_dac_decode_backward(hd, P(flat), v, P(tape), floats, P(audio), B, T, P(dzz), st), -1)
    for call in (lambda: lib.escx_dac_encode_tape_floats(hd, B, L, n), lambda: fwd(tape, floats), lambda: bwd(v, tape, floats)):       # padding off
        _native.check(lib.escx_dac_set_padding(hd, 0))
        try:
            rc = call()
        finally:
            _native.check(lib.escx_dac_set_padding(hd, 1))
        refused(rc, -2)
    _native.check(bwd(v, tape, floats))
    torch.cuda.synchronize()
    assert torch.equal(dx, want)
    # NULL cotangents are zeros
    _native.check(lib.escx_dac_encode_backward(hd, P(flat), v, P(tape), floats, None, None, None, B, L, P(dx), st))
    torch.cuda.synchronize()
    assert bool((dx == 0).all())
