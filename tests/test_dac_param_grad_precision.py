"""The split-operand weight gradients of esc.baselines.DAC (set_param_grad_precision("bf16x3"), include/escx.h
escx_dac_set_param_grad_precision) on the MI355X: the dW contraction of every decoder convolution with more than one input and output channel as
gemm_dw_bf16_kernel<DacConvA, DacConvA, 3> (128 x 128 tiles, three exact bf16 terms per operand, six cross products in fp32) or, where
Np <= 64 (all of dac_syn), dac_dw_x3_kernel's 64 x 128 and 32 x 128 tiles; dac_tiny and dac_base reach all three.  The guarantees
are the fp32 path's own (tests/test_dac_param_grad.py), whose cases, oracle (the REAL reference's fixture where it stores the tensor, the float64
restatement elsewhere), models and rule (dac_param_grad_util.check_rule) are shared by import, so every reference is computed once per session.

Measured on an MI355X (err_dev / err_eager per kind and shape): see DESIGN.md section 13.5."""
import ctypes

import pytest
import torch

import dac_grad_util as gu
import dac_param_grad_util as pu
import test_dac_param_grad as base
from test_dac_param_grad import _case, _dev, _fresh, _model, _np, _run

pytestmark = pytest.mark.gpu
PAIRS = (("fp32", "fp32"), ("bf16x3", "bf16x3"))               # (forward, input-gradient) modes the new mode is run under
SHAPES = [("dac_syn", 3, 7), ("dac_tiny", 2, 5), ("dac_tiny", 1, 1), ("dac_syn", 3, 37), ("dac_base", 1, 3)]


class _modes:
    """The three switches of a shared model for the length of a block; fp32 again behind it."""

    def __init__(self, m, fwd="fp32", grad="fp32", param="bf16x3"):
        self.m, self.want = m, (fwd, grad, param)

    def __enter__(self):
        self.m.set_precision(self.want[0]).set_grad_precision(self.want[1]).set_param_grad_precision(self.want[2])
        return self.m

    def __exit__(self, *exc):
        self.m.set_precision("fp32").set_grad_precision("fp32").set_param_grad_precision("fp32")


def _clone(grads):
    return {k: v.clone() for k, v in grads.items()}


def _one_channel(m):
    """The weight keys of the decoder's one-channel convolutions: they keep the fp32 kernel in every mode."""
    return [k for k, p in base._decoder_named(m).items() if pu.kind(k) in ("weight_v", "weight_g") and p.shape[0] == 1]


@pytest.mark.parametrize("fwd,grad", PAIRS)
@pytest.mark.parametrize("name,B,T", SHAPES)
def test_parameter_gradients_against_float64(name, B, T, fwd, grad):
    z, w, g64, err_eager = _case(name, B, T)
    with _modes(_model(name), fwd, grad) as m:
        audio, dz, grads = _run(m, z, w)
        with torch.no_grad():
            assert torch.equal(audio, m.decode(_dev(z))), "the parameter path's audio is not bitwise decode's"
    assert list(grads) == list(g64), "not exactly the decoder's parameters got a gradient"
    assert dz is not None and dz.shape == z.shape
    pu.check_rule(pu.errors(_np(grads), g64), err_eager, f"{name} {B}x{T} fwd/grad {fwd} param bf16x3")


def test_slices_of_the_128_tiles_and_todays_counts_in_fp32():
    """dac_syn at 3 x 37 under the new rule (256-row minimum, multiples of 32): the 444-row contractions of the last block run two slices of 224
    and 220 rows, the 111- and 222-row ones a single slice; the one-channel last layer keeps the fp32 rule's count.  In fp32 mode the query
    returns what tests/test_dac_param_grad.py pins."""
    m = _model("dac_syn")
    lib, hd, _, _, _ = m._ctx(torch.zeros(1, device="cuda"), "z")
    n_layers = 2 + 7 * len(m.decoder_rates)
    query = lambda: [lib.escx_dac_param_grad_slices(hd, 3, 37, i) for i in range(n_layers)]      # noqa: E731
    today = query()
    assert all(s == 1 for s in today[:2]) and all(s == 2 for s in today[2:9]) and all(s == 4 for s in today[9:])
    with _modes(m):
        new = query()
        print("slices per decoder layer at 3 x 37: fp32", today, "bf16x3", new)
        assert new[:9] == [1] * 9 and new[9:-1] == [2] * (n_layers - 10), new
        rows, per = 444, 224                                    # 444 rows in two slices of rup(222, 32) = 224: the last one has 220
        assert per % 32 == 0 and 0 < rows - per < per
        assert new[-1] == today[-1], "the one-channel layer left the fp32 rule"
        assert lib.escx_dac_param_grad_slices(hd, 3, 37, n_layers) == 0 and lib.escx_dac_param_grad_slices(hd, 3, 0, 0) == 0
    assert query() == today


@pytest.mark.parametrize("fwd,grad", PAIRS)
def test_the_kernel_ran_and_nothing_else_moved(fwd, grad):
    name, B, T = "dac_syn", 3, 37
    z, w = gu.inputs(name, B, T)
    m = _model(name)
    with _modes(m, fwd, grad, "fp32"):
        audio0, dz0, g0 = _run(m, z, w)
        g0 = _clone(g0)
    with _modes(m, fwd, grad):
        audio1, dz1, g1 = _run(m, z, w)
        g1 = _clone(g1)
        _, dz2, g2 = _run(m, z, w)
        assert torch.equal(dz1, dz2) and all(torch.equal(g1[k], g2[k]) for k in g1), "two backward calls differ"
        _, _, acc = _run(m, z, w, keep=True)                    # p.grad still holds the run before: autograd adds
        assert all(torch.equal(acc[k], 2 * g1[k]) for k in g1), "two accumulated backwards are not twice one"
    assert torch.equal(audio0, audio1) and torch.equal(dz0, dz1), "the audio or d_z depends on the weight gradients' mode"
    assert list(g0) == list(g1)
    moved = [k for k in g0 if not torch.equal(g0[k], g1[k])]
    print(f"{len(moved)} of {len(g0)} gradients differ in some bit between the modes")
    assert any(pu.kind(k) == "weight_v" for k in moved), "no weight_v gradient moved: the split-operand kernel did not run"
    assert all(pu.kind(k) in ("weight_v", "weight_g") for k in moved), "a bias or alpha gradient depends on the mode"
    one = _one_channel(m)
    assert len(one) == 2 and not set(one) & set(moved), "the one-channel layer left the fp32 kernel"


def test_zero_cotangent_gives_exactly_zero_gradients():
    name, B, T = "dac_syn", 3, 37
    z, w = gu.inputs(name, B, T)
    with _modes(_model(name)) as m:
        _, dz, grads = _run(m, z, 0.0 * w)
    assert len(grads) == len(base._decoder_named(m)) and all(not bool(g.any()) for g in grads.values()) and not bool(dz.any())


def test_mode_switches_on_one_handle_and_the_workspace():
    name, B, T = "dac_syn", 3, 37
    z, w = gu.inputs(name, B, T)
    m = _fresh(name).set_trainable("decoder")
    lib, hd, _, _, _ = m._ctx(torch.zeros(1, device="cuda"), "z")
    ws = lambda: int(lib.escx_dac_param_grad_workspace_floats(hd))      # noqa: E731
    w0 = ws()
    _, dz_a, a = _run(m, z, w)
    a = _clone(a)
    assert ws() == w0 > 0
    m.set_param_grad_precision("bf16x3")
    assert lib.escx_dac_get_param_grad_precision(hd) == 3
    assert ws() == w0, "the workspace grew before a backward ran in the mode"
    _, dz_b, b = _run(m, z, w)
    b = _clone(b)
    w1 = ws()
    assert w1 > w0, "the 128 x 128 tiles' partial region is not counted after the first backward in the mode"
    m.set_param_grad_precision("fp32")
    assert ws() == w0, "fp32 mode reports another workspace than before"
    _, dz_c, c = _run(m, z, w)
    assert torch.equal(dz_a, dz_b) and torch.equal(dz_a, dz_c)
    assert all(torch.equal(a[k], c[k]) for k in a), "fp32 -> bf16x3 -> fp32 does not give the first call's bits again"
    assert any(not torch.equal(a[k], b[k]) for k in a)
    m.set_param_grad_precision("bf16x3")
    assert ws() == w1
    _, _, b2 = _run(m, z, w)
    assert all(torch.equal(b[k], b2[k]) for k in b)


def test_three_optimiser_steps_in_the_mode():
    name, B, T = "dac_syn", 3, 7
    z, _ = gu.inputs(name, B, T)
    m = _fresh(name).set_trainable("decoder").set_param_grad_precision("bf16x3")
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
        got = {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}
        # a fresh model loaded from this step's state_dict: the same gradients, bit for bit (the re-pack and the refreshed images)
        twin = _fresh(name, sd).set_trainable("decoder").set_param_grad_precision("bf16x3")
        for k, p in twin.named_parameters():
            p.requires_grad_(k.startswith("decoder."))
        (twin.decode(zd) - td).pow(2).mean().backward()
        want = {k: p.grad for k, p in twin.named_parameters() if p.grad is not None}
        assert list(got) == list(want) and all(torch.equal(got[k], want[k]) for k in got), f"step {step}: gradients differ from a fresh model's"
        opt.step()
        with torch.no_grad():
            stepped = m.decode(zd)
        twin = _fresh(name, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
        assert torch.equal(stepped, twin.decode(zd)), f"step {step}: the stepped model decodes differently from a fresh model with its state_dict"
    print("losses:", losses)
    assert losses[2] < losses[0]


def test_python_refusals_are_unchanged_under_the_mode():
    z, w, _, _ = _case("dac_syn", 3, 7)
    m = _fresh().set_trainable("decoder").set_param_grad_precision("bf16x3")
    with torch.no_grad():
        before = m.decode(_dev(z))
    T = next(t for t in range(1, 400) if m._walk(t, m._conv_layers()[2 + 7 * len(m.encoder_rates):]) >= 1)
    m.padding = False
    try:
        with pytest.raises(NotImplementedError):
            m.decode(torch.zeros(1, m.latent_dim, T, device="cuda"))
    finally:
        m.padding = True
    m.train()
    with pytest.raises(NotImplementedError):
        m.decode(_dev(z))
    m.eval()
    for bad in ("f16x2", "nope"):
        with pytest.raises((NotImplementedError, ValueError)):
            m.set_param_grad_precision(bad)
    assert m.param_grad_precision == "bf16x3" and all(p.grad is None for p in m.parameters())
    with torch.no_grad():
        assert torch.equal(m.decode(_dev(z)), before), "the handle decodes differently after the refusals"


def test_c_level_refusals_and_the_other_slots_under_the_mode():
    from esc import _native
    z, w, _, _ = _case("dac_syn", 3, 7)
    m = _fresh().set_trainable("decoder").set_param_grad_precision("bf16x3")
    zc, wc = _dev(z), _dev(w).contiguous()
    with torch.no_grad():
        before = m.decode(zc)
    _, want_dz, want = _run(m, z, w)
    lib, hd, flat, dev, st = m._ctx(zc, "z")
    assert lib.escx_dac_set_param_grad_precision(hd, _native.PRECISIONS["f16x2"]) == -2 and lib.escx_dac_set_param_grad_precision(hd, 7) == -1
    assert lib.escx_dac_get_param_grad_precision(hd) == _native.PRECISIONS["bf16x3"], "a refused mode changed the handle"
    B, D, T = zc.shape
    P = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    v = m._version()
    floats = lib.escx_dac_decode_tape_floats(hd, B, T)
    tape, audio = torch.empty(floats, device="cuda"), torch.empty_like(before)
    _native.check(lib.escx_dac_decode_tape(hd, P(flat), v, P(zc), B, T, P(audio), P(tape), floats, st))
    layout = m._flat[dev.index if dev.index is not None else torch.cuda.current_device()]["layout"]
    first = min(off for k, off, n in layout if k.startswith("decoder."))
    assert first > 0 and layout[-1][1] + layout[-1][2] == flat.numel()
    grad, dz = torch.full_like(flat, 7.0), torch.full((B, D, T), 7.0, device="cuda")
    call = lambda ver, tp, gg: lib.escx_dac_decode_backward_params(hd, P(flat), ver, P(tp), floats, P(zc), P(wc), B, T, P(dz), gg, st)      # noqa: E731
    assert call(v + 1, tape, P(grad)) == -4 and b"version" in lib.escx_last_error()                            # a stale parameter version
    assert call(v, torch.zeros(floats, device="cuda"), P(grad)) == -1                                          # a foreign tape
    _native.check(lib.escx_dac_set_padding(hd, 0))
    try:
        assert call(v, tape, P(grad)) == -2
    finally:
        _native.check(lib.escx_dac_set_padding(hd, 1))
    torch.cuda.synchronize()
    assert bool((grad == 7.0).all()) and bool((dz == 7.0).all()), "a refused backward wrote an output"
    with torch.no_grad():
        assert torch.equal(m.decode(zc), before), "the handle decodes differently after the refused calls"
    assert call(v, tape, P(grad)) == 0
    torch.cuda.synchronize()
    assert bool((grad[:first] == 7.0).all()), "a float outside the decoder's slots was written"
    assert torch.equal(dz, want_dz)
    for k, off, n in layout:
        if k.startswith("decoder."):
            assert torch.equal(grad[off:off + n], want[k].reshape(-1)), k
