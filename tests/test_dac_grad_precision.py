"""The split-operand backward of the DAC baseline codec on the MI355X (DAC.set_grad_precision("bf16x3"), include/escx.h
escx_dac_set_grad_precision): the input gradient of every convolution of the decoder and the encoder on v_mfma_f32_16x16x32_bf16 with two-level
accumulation (csrc/dac_x3.h).  The accuracy rule, the oracles and the cases are those of test_dac_grad.py, test_dac_encode_grad.py and
test_dac_param_grad.py (whose helpers and cached float64 references are shared): err_dev <= 2 * err_eager against float64, with err_eager the
float32 torch-eager error of the same case, and the per-kind rms rule for the parameter gradients.

What each case reaches in the backward's launcher (csrc/dac.hip launch_grad / csrc/dac_x3.h launch_dac_x3; Np = rup(Cin, 16), Kp = rup(K cpad(Cout), 16),
chunk = dac_x3_chunk(Kp) steps of 32 per restart of the MFMA chain):
  64 x 32 tile                  every dac_syn case; dac_tiny decoder width 18, encoder width 32
  64 x 64                       dac_tiny decoder width 36 (Np 48), encoder width 64; dac_base encoder width 64
  64 x 96                       dac_tiny decoder widths 288, 144, 72 (Np 80); dac_base decoder widths 192, 96
  64 x 128                      dac_tiny decoder's first convolution (Np 512), encoder widths 128 ... 512; dac_base widths 1536 ... 384
  128-row tiles (>= 512 tiles)  none of the listed cases.  Added: dac_syn 1 x 16353 frames (128 x 32: 65412 rows at width 8, 511 full tiles and one of
                                4 rows) and dac_syn 1 x 65412 samples for the encoder.  128 x 64 needs a wider model: test_wide_batch_of_dac_base
                                (encoder width 64 at 176000 rows).  The backward has no 128 x 96 and 128 x 128 tile (csrc/dac_x3.h: registers);
                                the same test runs those widths on many 64-row tiles (decoder widths 192, 96 and 384 at 88000, 176000 and 22000 rows)
  Kp not a multiple of 32       every dac_syn case (Kp 16, 48, 112, 224) and dac_tiny's decoder (Kp 144: width 36 one-tap, ...); never dac_base
  rows not a multiple of tile   every case but dac_syn 2 x 96 and 8 x 24 (768 rows)
  chunk 1 / 2 / 4 / 8           dac_syn: 1 only; dac_tiny: 1, 2; dac_base 1 x 3: 1, 2, 4 (Kp 3840, 5376, 10752) and 8 (Kp 12288, the first
                                DecoderBlock's ConvTranspose1d); dac_base encoder: 1, 2, 4
  short last chunk              dac_tiny (Kp 2016 = 63 steps, chunk 2); dac_base Kp 5376 = 168 steps is whole, Kp 672 = 21 steps runs chunk 1
  two-slice branch of dW        dac_syn 3 x 37 (fp32 contraction in both grad modes; its operands come from the bf16x3 input gradients here)
  fp32 MFMA under the mode      the one-channel layers (decoder's last, encoder's first convolution) in every case, as in the forward mode

Measured on an MI355X: see DESIGN.md sections 13.3 - 13.5."""
import ctypes

import numpy as np
import pytest
import torch

import dac_encode_grad_util as eu
import dac_grad_util as gu
import dac_param_grad_util as pu
import test_dac_encode_grad as te
import test_dac_grad as tg
import test_dac_param_grad as tp

pytestmark = pytest.mark.gpu
MODES = ("fp32", "bf16x3")
_dev = tg._dev


class _modes:
    """A shared model in (forward mode, grad mode) for the length of a with block; both are put back to fp32."""

    def __init__(self, m, fwd, grad):
        self.m, self.fwd, self.grad = m, fwd, grad

    def __enter__(self):
        self.m.set_precision(self.fwd).set_grad_precision(self.grad)
        return self.m

    def __exit__(self, *exc):
        self.m.set_precision("fp32").set_grad_precision("fp32")


# ---- accuracy against float64 ---------------------------------------------------------------------------------------------------------------
LATENT_CASES = [("dac_syn", 3, 7), ("dac_syn", 1, 1), ("dac_syn", 2, 96), ("dac_tiny", 2, 5), ("dac_tiny", 1, 1), ("dac_base", 1, 3), ("dac_syn", 1, 16353)]


@pytest.mark.parametrize("fwd", MODES)
@pytest.mark.parametrize("name,B,T", LATENT_CASES)
def test_latent_gradient_against_float64(name, B, T, fwd):
    z, w, d64, err_eager = tg._case(name, B, T)
    with _modes(tg._model(name), fwd, "bf16x3") as m:
        audio, dz = tg._grad(m, z, w)
        m.set_grad_precision("fp32")
        assert torch.equal(audio, m.decode(_dev(z))), "the audio depends on the grad mode"
    assert dz.shape == d64.shape and dz.dtype == torch.float32
    err_dev = gu.rel_l2(dz.cpu().numpy(), d64)
    print(f"{name} {B}x{T} fwd {fwd} grad bf16x3: err_dev {err_dev:.3e}  err_eager {err_eager:.3e}  ratio {err_dev / err_eager:.2f}")
    assert 1e-8 < err_eager < 5e-6, err_eager
    assert err_dev <= 2 * err_eager, (err_dev, err_eager)


@pytest.mark.parametrize("fwd", MODES)
@pytest.mark.parametrize("name,B,L,n", te.CASES + [("dac_syn", 1, 65412, 2)])
def test_audio_gradient_against_float64(name, B, L, n, fwd):
    x, cot = eu.inputs(name, B, L, n)
    with _modes(te._model(name), fwd, "bf16x3") as m:
        got, dx = te._grad(m, x, cot, n)
        m.set_grad_precision("fp32")
        te._same_values(got, m.encode(_dev(x), n))
    d64, err_eager = te._oracles(name, B, L, n, got[1].cpu().numpy().tobytes())
    te._rule(f"{name} {B}x{L} n{n} fwd {fwd} grad bf16x3", dx, d64, err_eager)


@pytest.mark.parametrize("fwd", MODES)
def test_audio_gradient_with_per_clip_counts(fwd):
    name, B, L, n = "dac_syn", 3, 28, 4
    counts = [1, 4, 2]
    x, cot = eu.inputs(name, B, L, n)
    with _modes(te._model(name), fwd, "bf16x3") as m:
        got, dx = te._grad(m, x, cot, counts)
    d64, err_eager = te._oracles(name, B, L, n, got[1].cpu().numpy().tobytes(), counts=tuple(counts))
    te._rule(f"{name} {B}x{L} per-clip {counts} fwd {fwd} grad bf16x3", dx, d64, err_eager)


@pytest.mark.parametrize("fwd", MODES)
@pytest.mark.parametrize("name,B,T", [("dac_syn", 3, 7), ("dac_tiny", 2, 5), ("dac_tiny", 1, 1), ("dac_syn", 3, 37), ("dac_base", 1, 3)])
def test_parameter_gradients_against_float64(name, B, T, fwd):
    z, w, g64, err_eager = tp._case(name, B, T)
    with _modes(tp._model(name), fwd, "bf16x3") as m:
        _, dz, grads = tp._run(m, z, w)
    assert list(grads) == list(g64) and dz is not None and dz.shape == z.shape
    pu.check_rule(pu.errors(tp._np(grads), g64), err_eager, f"{name} {B}x{T} fwd {fwd} grad bf16x3")


# ---- bitwise properties (dac_syn) -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fwd", MODES)
def test_forward_values_determinism_and_batch_independence(fwd):
    name, B, T = "dac_syn", 8, 24
    z, w = gu.inputs(name, B, T)
    with _modes(tg._model(name), fwd, "fp32") as m:
        audio32, _ = tg._grad(m, z, w)
        m.set_grad_precision("bf16x3")
        audio, dz = tg._grad(m, z, w)
        assert torch.equal(audio, audio32), "decode's output depends on the grad mode"
        _, again = tg._grad(m, z, w)
        assert torch.equal(dz, again), "two backward calls differ"
        for i in (0, 3, 7):
            _, one = tg._grad(m, z[i:i + 1], w[i:i + 1])
            assert torch.equal(one, dz[i:i + 1]), i
    L, n = 96, 4
    x, cot = eu.inputs(name, B, L, n)
    cot = {k: cot[k] for k in ("z", "latents")}          # the commitment mean carries 1 / B of the call
    with _modes(te._model(name), fwd, "fp32") as m:
        got32, _ = te._grad(m, x, cot, n)
        m.set_grad_precision("bf16x3")
        got, dx = te._grad(m, x, cot, n)
        assert all(torch.equal(a, b) for a, b in zip(got, got32)), "encode's outputs depend on the grad mode"
        _, again = te._grad(m, x, cot, n)
        assert torch.equal(dx, again), "two backward calls differ"
        for i in (0, 3, 7):
            _, one = te._grad(m, x[i:i + 1], {k: v[i:i + 1] for k, v in cot.items()}, n)
            assert torch.equal(one, dx[i:i + 1]), i


@pytest.mark.parametrize("fwd", MODES)
def test_trainable_decoder_gives_the_latent_only_d_z(fwd):
    name, B, T = "dac_syn", 3, 37
    z, w = gu.inputs(name, B, T)
    with _modes(tp._model(name), fwd, "bf16x3") as m:
        _, dz, g1 = tp._run(m, z, w)
        g1 = {k: v.clone() for k, v in g1.items()}
        _, dz2, g2 = tp._run(m, z, w)
        assert torch.equal(dz, dz2) and all(torch.equal(g1[k], g2[k]) for k in g1), "two backward calls differ"
    with _modes(tg._model(name), fwd, "bf16x3") as m:
        _, want = tg._grad(m, z, w)
    assert torch.equal(dz, want), "z.grad under set_trainable('decoder') differs from the latent-only path's"


def test_zero_cotangents_give_exact_zeros():
    name = "dac_syn"
    z, w, _, _ = tg._case(name, 2, 96)
    with _modes(tg._model(name), "fp32", "bf16x3") as m:
        _, dz = tg._grad(m, z, np.zeros_like(w))
    assert np.array_equal(dz.cpu().numpy(), np.zeros(z.shape, np.float32))
    x, cot = eu.inputs(name, 2, 1027, 3)
    with _modes(te._model(name), "fp32", "bf16x3") as m:
        _, dx = te._grad(m, x, {k: np.zeros_like(v) for k, v in cot.items()}, 3)
    assert np.array_equal(dx.cpu().numpy(), np.zeros(x.shape, np.float32))


@pytest.mark.parametrize("where", ("first", "middle", "last"))
def test_one_sample_cotangent_keeps_the_exact_zeros(where):
    name, B, T = "dac_syn", 2, 96
    z, _, _, _ = tg._case(name, B, T)
    n = gu.du.output_samples(gu.config(name), T)
    w = np.zeros((B, 1, n))
    w[0, 0, {"first": 0, "middle": n // 2, "last": n - 1}[where]] = 1.0
    d64 = gu.oracle(name, z, w)
    zero = d64 == 0
    assert zero[1].all() and 0 < int(zero[0].sum()) < zero[0].size, "the oracle's support does not exercise the check"
    with _modes(tg._model(name), "fp32", "bf16x3") as m:
        _, dz = tg._grad(m, z, w)
    dz = dz.cpu().numpy()
    assert np.array_equal(dz[zero], np.zeros(int(zero.sum()), np.float32)), "nonzero where the float64 oracle is exactly zero"
    assert np.array_equal(dz[1], np.zeros_like(dz[1]))
    assert gu.rel_l2(dz, d64) < 1e-5


@pytest.mark.parametrize("t", (0, 128, 255))
def test_one_frame_cotangent_keeps_the_exact_zeros_of_d_audio(t):
    name, B, L, n = "dac_syn", 2, 1027, 3
    x, _ = eu.inputs(name, B, L, n)
    D, T, n, d = eu.shapes(name, B, L, n)
    w = np.zeros((B, D, T))
    w[0, :, t] = 1.0
    with _modes(te._model(name), "fp32", "bf16x3") as m:
        got, dx = te._grad(m, x, {"z": w}, n)
    d64 = eu.oracle(name, x, {"z": w}, n, codes=got[1].cpu().numpy())
    zero = d64 == 0
    assert zero[1].all() and 0 < int(zero[0].sum()) < zero[0].size, "the oracle's support does not exercise the check"
    dx = dx.cpu().numpy()
    assert np.array_equal(dx[zero], np.zeros(int(zero.sum()), np.float32)), "nonzero where the float64 oracle is exactly zero"
    assert eu.rel_l2(dx, d64) < 1e-5


def test_two_graphs_alive_backwarded_in_reverse_order():
    name = "dac_syn"
    z1, w1, _, _ = tg._case(name, 3, 7)
    z2, w2 = gu.inputs(name, 2, 5)
    with _modes(tg._model(name), "fp32", "bf16x3") as m:
        _, solo1 = tg._grad(m, z1, w1)
        _, solo2 = tg._grad(m, z2, w2)
        a, b = _dev(z1).requires_grad_(True), _dev(z2).requires_grad_(True)
        out_a, out_b = m.decode(a), m.decode(b)
        (out_b * _dev(w2)).sum().backward()
        (out_a * _dev(w1)).sum().backward()
        assert torch.equal(a.grad, solo1) and torch.equal(b.grad, solo2)


# ---- the mode is really in use --------------------------------------------------------------------------------------------------------------
def test_bf16x3_backward_is_another_summation_order():
    name, B, T = "dac_syn", 2, 96
    z, w, d64, err_eager = tg._case(name, B, T)
    with _modes(tg._model(name), "fp32", "fp32") as m:
        _, d32 = tg._grad(m, z, w)
        m.set_grad_precision("bf16x3")
        _, d16 = tg._grad(m, z, w)
    assert not torch.equal(d32, d16), "the bf16x3 backward gave the fp32 backward's bits: is the mode in use?"
    for tag, d in (("fp32", d32), ("bf16x3", d16)):
        err = gu.rel_l2(d.cpu().numpy(), d64)
        print(f"{name} {B}x{T} grad {tag}: err_dev {err:.3e}  err_eager {err_eager:.3e}  ratio {err / err_eager:.2f}")
        assert err <= 2 * err_eager, (tag, err, err_eager)


# ---- mode switching and parameter changes ---------------------------------------------------------------------------------------------------
def _change(m):
    with torch.no_grad():
        m.get_parameter("encoder.block.1.block.0.block.1.weight_g").mul_(1.5)
        m.get_parameter("decoder.model.1.block.2.block.1.weight_g").mul_(1.5)
        m.get_parameter("decoder.model.1.block.0.alpha").add_(0.25)


def test_mode_round_trip_and_parameter_change_rebuild_the_mirrors():
    name = "dac_syn"
    z, w, _, _ = tg._case(name, 3, 7)
    x, cot = eu.inputs(name, 3, 28, 4)
    m = tg._fresh(name)
    _, first = tg._grad(m, z, w)
    _, first_x = te._grad(m, x, cot, 4)
    m.set_grad_precision("bf16x3")
    _, mid = tg._grad(m, z, w)
    _, mid_x = te._grad(m, x, cot, 4)
    m.set_grad_precision("fp32")
    _, last = tg._grad(m, z, w)
    _, last_x = te._grad(m, x, cot, 4)
    assert torch.equal(first, last) and torch.equal(first_x, last_x), "fp32 after a round trip through bf16x3 is not the first result"
    # a parameter change between two bf16x3 backwards: the mirrors follow the transposed images
    m.set_grad_precision("bf16x3")
    _change(m)
    _, after = tg._grad(m, z, w)
    _, after_x = te._grad(m, x, cot, 4)
    assert not torch.equal(after, mid) and not torch.equal(after_x, mid_x)
    twin = tg._fresh(name)
    twin.load_state_dict({k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, strict=True)
    twin = twin.cuda().eval().set_grad_precision("bf16x3")
    _, want = tg._grad(twin, z, w)
    _, want_x = te._grad(twin, x, cot, 4)
    assert torch.equal(after, want) and torch.equal(after_x, want_x), "a handle that held older mirrors differs from a fresh one"
    # the change made while the handle ran in fp32, then the switch: the mirrors must still be the current parameters'
    m.set_grad_precision("fp32")
    _change(m)
    tg._grad(m, z, w)
    te._grad(m, x, cot, 4)
    m.set_grad_precision("bf16x3")
    _, got = tg._grad(m, z, w)
    _, got_x = te._grad(m, x, cot, 4)
    _change(twin)
    _, want = tg._grad(twin, z, w)
    _, want_x = te._grad(twin, x, cot, 4)
    assert torch.equal(got, want) and torch.equal(got_x, want_x)


# ---- error paths ----------------------------------------------------------------------------------------------------------------------------
def test_abi_set_get_and_refusals():
    from esc import _native
    m = tg._fresh()
    lib, hd = m._handle(torch.device("cuda:0"))
    assert lib.escx_dac_get_grad_precision(hd) == _native.PRECISIONS["fp32"] == 0
    assert lib.escx_dac_set_grad_precision(hd, _native.PRECISIONS["bf16x3"]) == 0 and lib.escx_dac_get_grad_precision(hd) == 3
    assert lib.escx_dac_get_precision(hd) == 0, "the grad mode moved the forward mode"
    assert lib.escx_dac_set_grad_precision(hd, _native.PRECISIONS["f16x2"]) == _native.ESCX_ERR_UNSUPPORTED
    assert lib.escx_dac_set_grad_precision(hd, 7) == _native.ESCX_ERR_INVALID_ARG and lib.escx_dac_set_grad_precision(hd, -1) == _native.ESCX_ERR_INVALID_ARG
    assert lib.escx_dac_get_grad_precision(hd) == 3                 # refusals leave the mode alone
    assert lib.escx_dac_set_precision(hd, 3) == 0 and lib.escx_dac_get_grad_precision(hd) == 3
    assert lib.escx_dac_set_grad_precision(hd, 0) == 0 and lib.escx_dac_get_grad_precision(hd) == 0 and lib.escx_dac_get_precision(hd) == 3
    assert lib.escx_dac_set_grad_precision(None, 0) == _native.ESCX_ERR_INVALID_ARG and lib.escx_dac_get_grad_precision(None) == -1
    # the setter before any handle exists, and every live handle follows it
    mm = tg._fresh().cpu().set_grad_precision("bf16x3").cuda()
    assert lib.escx_dac_get_grad_precision(mm._handle(torch.device("cuda:0"))[1]) == 3 and mm.grad_precision == "bf16x3"
    mm.set_grad_precision("fp32")
    assert lib.escx_dac_get_grad_precision(mm._handle(torch.device("cuda:0"))[1]) == 0


def test_python_errors_leave_the_handle_usable_and_the_mode_unchanged():
    z, w, _, _ = tg._case("dac_syn", 3, 7)
    m = tg._fresh().set_grad_precision("bf16x3")
    _, want = tg._grad(m, z, w)
    # padding off
    T = next(t for t in range(1, 400) if m._walk(t, m._conv_layers()[2 + 7 * len(m.encoder_rates):]) >= 1)
    m.padding = False
    try:
        with pytest.raises(NotImplementedError):
            m.decode(torch.zeros(1, m.latent_dim, T, device="cuda").requires_grad_(True))
    finally:
        m.padding = True
    # double backward
    zt = _dev(z).requires_grad_(True)
    (g,) = torch.autograd.grad((m.decode(zt) * _dev(w)).sum(), zt, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    # training mode
    m.train()
    with pytest.raises(NotImplementedError):
        m.decode(_dev(z).requires_grad_(True))
    m.eval()
    assert m.grad_precision == "bf16x3"
    _, again = tg._grad(m, z, w)
    assert torch.equal(again, want), "the handle differentiates differently after the refused calls"
    # changed parameters between forward and backward
    zt = _dev(z).requires_grad_(True)
    out = m.decode(zt)
    with torch.no_grad():
        m.get_parameter("decoder.model.1.block.0.alpha").add_(0.25)
    with pytest.raises(RuntimeError, match="changed in place"):
        (out * _dev(w)).sum().backward()
    assert zt.grad is None and m.grad_precision == "bf16x3"
    tg._grad(m, z, w)


def test_c_level_errors_in_the_new_mode():
    from esc import _native
    z, w, _, _ = tg._case("dac_syn", 3, 7)
    m = tg._fresh().set_grad_precision("bf16x3")
    zc, wc = _dev(z), _dev(w).contiguous()
    _, want = tg._grad(m, z, w)
    lib, hd, flat, dev, st = m._ctx(zc, "z")
    B, D, T = zc.shape
    P = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    v = m._version()
    floats = lib.escx_dac_decode_tape_floats(hd, B, T)
    tape, audio, dz = torch.empty(floats, device="cuda"), torch.empty(B, 1, gu.du.output_samples(gu.config("dac_syn"), T), device="cuda"), torch.full((B, D, T), 7.0, device="cuda")
    _native.check(lib.escx_dac_decode_tape(hd, P(flat), v, P(zc), B, T, P(audio), P(tape), floats, st))
    assert lib.escx_dac_decode_backward(hd, P(flat), v + 1, P(tape), floats, P(wc), B, T, P(dz), st) == -4                         # a stale parameter version
    assert lib.escx_dac_decode_backward(hd, P(flat), v, P(torch.zeros(floats, device="cuda")), floats, P(wc), B, T, P(dz), st) == -1     # not a tape
    _native.check(lib.escx_dac_set_padding(hd, 0))
    try:
        assert lib.escx_dac_decode_backward(hd, P(flat), v, P(tape), floats, P(wc), B, T, P(dz), st) == -2
    finally:
        _native.check(lib.escx_dac_set_padding(hd, 1))
    torch.cuda.synchronize()
    assert bool((dz == 7.0).all()), "a refused backward wrote its output"
    assert lib.escx_dac_get_grad_precision(hd) == 3
    # a tape is valid under either mode: made above under bf16x3's handle, backwarded in fp32 and then in bf16x3
    _native.check(lib.escx_dac_set_grad_precision(hd, 0))
    _native.check(lib.escx_dac_decode_backward(hd, P(flat), v, P(tape), floats, P(wc), B, T, P(dz), st))
    torch.cuda.synchronize()
    m32 = tg._model("dac_syn")
    _, want32 = tg._grad(m32, z, w)
    assert torch.equal(dz, want32)
    _native.check(lib.escx_dac_set_grad_precision(hd, 3))
    _native.check(lib.escx_dac_decode_backward(hd, P(flat), v, P(tape), floats, P(wc), B, T, P(dz), st))
    torch.cuda.synchronize()
    assert torch.equal(dz, want)


# ---- the 128-row tiles of every column width ------------------------------------------------------------------------------------------------
def test_wide_batch_of_dac_base():
    """Eleven 1 s clips through DAC-Base (the module docstring lists the tiles): under bf16x3 a clip's d_z and d_audio in the batch (128-row tiles
    where the launcher has them, hundreds of workgroups elsewhere) are bitwise the clip's alone, and both gradients agree with the fp32 backward of
    the same graph within 1e-5, the bound the sibling tests use for two fp32-grade results of the same sum (20 x the float32 error of the reference
    itself); they must also differ, or the mode was not in use."""
    name, B, T = "dac_base", 11, 50
    m = tg._model(name)
    g = torch.Generator().manual_seed(20)
    z = torch.rand(B, m.latent_dim, T, generator=g).mul_(2).sub_(1).numpy()
    L = T * 320
    w = torch.rand(B, 1, gu.du.output_samples(gu.du.full_config(gu.config(name)), T), generator=g).mul_(2).sub_(1).numpy()
    with _modes(m, "fp32", "fp32"):
        _, d32 = tg._grad(m, z, w)
        m.set_grad_precision("bf16x3")
        _, dz = tg._grad(m, z, w)
        for i in (0, 10):
            _, one = tg._grad(m, z[i:i + 1], w[i:i + 1])
            assert torch.equal(one, dz[i:i + 1]), i
    rel = gu.rel_l2(dz.cpu().numpy(), d32.cpu().numpy())
    print(f"DAC-Base {B} x {T} frames: d_z bf16x3 against fp32 {rel:.3e}")
    assert 0 < rel < 1e-5
    x = torch.rand(B, 1, L, generator=g).sub_(0.5).numpy()
    cz = torch.rand(B, m.latent_dim, eu.shapes(name, B, L, 18)[1], generator=g).mul_(2).sub_(1).numpy()
    with _modes(m, "fp32", "fp32"):
        _, x32 = te._grad(m, x, {"z": cz}, 18)
        m.set_grad_precision("bf16x3")
        _, dx = te._grad(m, x, {"z": cz}, 18)
        for i in (0, 10):
            _, one = te._grad(m, x[i:i + 1], {"z": cz[i:i + 1]}, 18)
            assert torch.equal(one, dx[i:i + 1]), i
    rel = eu.rel_l2(dx.cpu().numpy(), x32.cpu().numpy())
    print(f"DAC-Base {B} x {L} samples: d_audio bf16x3 against fp32 {rel:.3e}")
    assert 0 < rel < 1e-5
