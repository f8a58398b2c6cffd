"""The encoder's and the quantiser's parameter gradients of esc.baselines.DAC.encode after set_encode_trainable on the MI355X (include/escx.h
escx_dac_encode_backward_params) against float64: the REAL reference's fixture (tools/gen_dac_encode_param_grad_golden.py) where it stores a
tensor in full, else the float64 restatement of tests/dac_encode_param_grad_util.py with the device's codes forced, which the host test pins to
the fixture.  Accuracy is measured per kind of parameter (bias, weight_g, weight_v, alpha, codebook) against the reference arithmetic's own
float32 error (torch eager on the CPU with the same codes forced), dac_encode_param_grad_util.check_rule: rms(err_dev) <= 2 rms(err_eager) and
every tensor's err_dev <= 2 max(err_eager) of its kind, each eager error taken no lower than 2^-24.

Measured on an MI355X (err_dev / err_eager per kind and shape): see DESIGN.md section 13.7."""
import ctypes

import numpy as np
import pytest
import torch

import dac_encode_grad_util as eu
import dac_encode_param_grad_util as qu
from conftest import load_golden

pytestmark = pytest.mark.gpu
MODES = ("fp32", "bf16x3")
_MODELS, _TRUTH = {}, {}
# (name, B, L, n, per-clip counts): what each shape alone reaches is in DESIGN.md section 13.7
CASES = [("dac_syn", 3, 28, 4, None), ("dac_syn", 1, 4, 4, None), ("dac_syn", 2, 1027, 3, None), ("dac_tiny", 2, 1600, 18, None),
         ("dac_tiny", 1, 335, 5, None), ("dac_base", 1, 960, 18, None), ("dac_syn", 3, 28, 4, (1, 4, 2))]


def _fresh(name="dac_syn", sd=None):
    from esc.baselines import DAC
    m = DAC(**eu.config(name))
    m.load_state_dict(eu.state_dict(name) if sd is None else sd, strict=True)
    return m.cuda().eval()


def _model(name):
    """One model per configuration with encode's switch on "both"; a test that changes its switches puts them back."""
    if name not in _MODELS:
        _MODELS[name] = _fresh(name).set_encode_trainable("both")
    return _MODELS[name]


def _dev(a):
    return torch.from_numpy(np.asarray(a, np.float32)).cuda()


def _np(grads):
    return {k: v.detach().cpu().numpy() for k, v in grads.items()}


def _encode_named(m):
    return {k: p for k, p in m.named_parameters() if k.startswith(("encoder.", "quantizer."))}


def _loss(out, cot):
    z, _, latents, cm, cb = out
    terms = {"z": z, "latents": latents, "cm": cm, "cb": cb}
    return sum((terms[k] * _dev(w)).sum() for k, w in cot.items())


def _run(m, x, cot, n, counts=None, want=None, x_grad=True, keep=False):
    """(encode's outputs detached, x.grad, {key: p.grad}) of sum_k sum(out[k] * cot[k]) on the device with the encoder / quantiser parameters in
    `want` (all by default) requiring gradients."""
    named = _encode_named(m)
    for k, p in m.named_parameters():
        p.requires_grad_(k in named and (want is None or k in want))
        if not keep:
            p.grad = None
    xt = _dev(x).requires_grad_(x_grad)
    out = m.encode(xt, n if counts is None else list(counts))
    assert out[0].grad_fn is not None and type(out[0].grad_fn).__name__.startswith("_EncodeParamGrad")
    _loss(out, cot).backward()
    torch.cuda.synchronize()
    return tuple(o.detach() for o in out), xt.grad, {k: p.grad for k, p in m.named_parameters() if p.grad is not None}


def _truth(name, B, L, n, counts, codes):
    """(g64 {key: float64 gradient or None}, err_eager {key: error of float32 eager}) for the codes the device chose: g64 is the fixture's tensor
    where it stores one in full, else the float64 restatement's with those codes forced; computed once per set of codes and left unchanged."""
    key = (name, B, L, n, counts, codes.tobytes())
    if key not in _TRUTH:
        x, cot = qu.inputs(name, B, L, n)
        g64 = qu.oracle(name, x, cot, n, codes=codes, counts=counts)
        if qu.FIXTURE_CASES.get(name) == (B, L, n) and counts is None:
            g = load_golden("dac_encode_param_grad")
            assert np.array_equal(codes, g[f"{name}_codes"]), f"{name}: the device's codes are not the reference's"
            g64 = qu.with_fixture(name, g64, g)
        eager = qu.oracle(name, x, cot, n, torch.float32, codes=codes, counts=counts)
        for a in g64.values():
            if a is not None:
                a.setflags(write=False)
        _TRUTH[key] = (g64, qu.errors(eager, g64))
    return _TRUTH[key]


def _check_case(m, name, B, L, n, counts, label):
    x, cot = qu.inputs(name, B, L, n)
    out, dx, grads = _run(m, x, cot, n, counts)
    with torch.no_grad():
        plain = m.encode(_dev(x), n if counts is None else list(counts))
    assert all(torch.equal(a, b) for a, b in zip(out, plain)), "the parameter path's forward values are not bitwise encode's"
    g64, err_eager = _truth(name, B, L, n, counts, out[1].cpu().numpy())
    named = _encode_named(m)
    assert list(g64) == list(named)
    assert [k for k in named if k not in grads] == [k for k, v in g64.items() if v is None], "not exactly the stages the call ran got a gradient"
    stages = max(counts) if counts else min(n, m.n_codebooks)
    assert all((qu.stage_of(k) is not None and qu.stage_of(k) >= stages) == (k not in grads) for k in named)
    for k, g in grads.items():
        assert g.shape == named[k].shape == g64[k].shape and g.dtype == torch.float32 and bool(g.ne(0).any()), k
    assert dx is not None and dx.shape == x.shape
    qu.check_rule(qu.errors(_np(grads), g64), err_eager, label)
    return out, dx, grads


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name,B,L,n,counts", CASES)
def test_parameter_gradients_against_float64(name, B, L, n, counts, mode):
    m = _model(name)
    m.set_precision(mode)
    try:
        out, _, grads = _check_case(m, name, B, L, n, counts, f"{name} {B}x{L} n{n}{'' if counts is None else list(counts)} {mode}")
    finally:
        m.set_precision("fp32")
    if (name, B, L) == ("dac_syn", 1, 4):                       # one frame, one row: every codebook row but the chosen one exactly zero
        for i in range(4):
            cb = grads[f"quantizer.quantizers.{i}.codebook.weight"]
            assert int(cb.ne(0).any(dim=1).sum()) == 1 and bool(cb[int(out[1][0, i, 0])].ne(0).any())
    if (name, B, L) == ("dac_syn", 2, 1027):                    # a row no code selects is exactly zero, every other one is not
        for i in range(3):
            cb = grads[f"quantizer.quantizers.{i}.codebook.weight"]
            used = torch.zeros(cb.shape[0], dtype=torch.bool, device="cuda").index_fill_(0, out[1][:, i].reshape(-1), True)
            assert torch.equal(cb.ne(0).any(dim=1), used)


@pytest.mark.parametrize("name,B,L,n", [("dac_syn", 2, 1027, 3), ("dac_tiny", 2, 1600, 18)])
def test_parameter_gradients_with_both_split_operand_grad_modes(name, B, L, n):
    m = _model(name)
    m.set_grad_precision("bf16x3").set_param_grad_precision("bf16x3")
    try:
        _check_case(m, name, B, L, n, None, f"{name} {B}x{L} n{n} grad bf16x3 + param grad bf16x3")
    finally:
        m.set_grad_precision("fp32").set_param_grad_precision("fp32")


def test_more_than_one_slice_a_ragged_last_slice_and_the_workspace():
    """dac_syn at 2 x 1027: the early layers' contractions run over 2054 rows, no multiple of the 128-row slice, in more than one slice; the first
    strided convolution's backward has an input row its phase GEMMs' taps do not cover (1027 is odd).  The workspace grows only once an encode
    parameter backward has run on the handle."""
    m = _fresh().set_encode_trainable("both")
    lib, hd, _, _, _ = m._ctx(torch.zeros(1, device="cuda"), "x")
    n_layers = 2 + 7 * len(m.encoder_rates)
    slices = [lib.escx_dac_encode_param_grad_slices(hd, 2, 1027, i) for i in range(n_layers)]
    print("slices per encoder layer at 2 x 1027:", slices)
    assert all(s >= 1 for s in slices) and slices[0] > 1 and slices[1] > 1 and (2 * 1027) % 128 != 0
    assert lib.escx_dac_encode_param_grad_slices(hd, 2, 1027, n_layers) == 0 and lib.escx_dac_encode_param_grad_slices(hd, 2, 0, 0) == 0
    before = lib.escx_dac_param_grad_workspace_floats(hd)
    x, cot = qu.inputs("dac_syn", 2, 1027, 3)
    _run(m, x, cot, 3)
    after = lib.escx_dac_param_grad_workspace_floats(hd)
    assert after > before > 0
    _run(m, x, cot, 3)
    assert lib.escx_dac_param_grad_workspace_floats(hd) == after


def test_forward_with_both_switches_gives_every_parameter_its_gradient():
    name, B, L = "dac_syn", 2, 30
    m = _fresh(name).set_encode_trainable("both").set_trainable("decoder")
    x = eu.seeded(f"x:forward:{name}:{B}x{L}", (B, 1, L), 0.5)
    w = eu.seeded(f"w_audio:forward:{name}:{B}x{L}", (B, 1, L))
    for p in m.parameters():
        p.requires_grad_(True)
    xt = _dev(x).requires_grad_(True)
    out = m(xt)
    (out["audio"] * _dev(w)).sum().backward()
    torch.cuda.synchronize()
    with torch.no_grad():
        plain = m(_dev(x))
    assert all(torch.equal(out[k].detach(), plain[k]) for k in plain), "the training path's forward values are not bitwise forward's"
    assert all(p.grad is not None for p in m.parameters()) and xt.grad is not None, "a parameter of the model got no gradient"
    codes = out["codes"].cpu().numpy()
    g64 = qu.oracle(name, x, {"audio": w}, codes=codes, whole=True)
    eager = qu.oracle(name, x, {"audio": w}, None, torch.float32, codes=codes, whole=True)
    got = _np({k: p.grad for k, p in m.named_parameters()})
    # the audio alone puts no codebook on the reference's graph (the straight-through estimator detaches it): exact zeros here
    off_graph = [k for k, v in g64.items() if v is None]
    assert off_graph == [k for k in g64 if qu.kind(k) == "codebook"] and all(not got[k].any() for k in off_graph)
    qu.check_rule(qu.errors(got, g64), qu.errors(eager, g64), f"forward {name} {B}x{L}")


@pytest.mark.parametrize("mode", MODES)
def test_bitwise_audio_gradient_determinism_and_accumulation(mode):
    name, B, L, n = "dac_syn", 2, 1027, 3
    x, cot = qu.inputs(name, B, L, n)
    m = _model(name)
    m.set_precision(mode)
    try:
        out, dx, g1 = _run(m, x, cot, n)
        g1 = {k: v.clone() for k, v in g1.items()}
        _, dx2, g2 = _run(m, x, cot, n)
        assert torch.equal(dx, dx2) and list(g1) == list(g2) and all(torch.equal(g1[k], g2[k]) for k in g1), "two backward calls differ"
        _, _, acc = _run(m, x, cot, n, keep=True)               # p.grad still holds the run before: autograd adds
        assert all(torch.equal(acc[k], 2 * g1[k]) for k in g1), "two accumulated backwards are not twice one"
        # frozen parameters fall back to the audio-only path: the same values and the same d_audio, bit for bit
        for p in m.parameters():
            p.requires_grad_(False)
            p.grad = None
        xt = _dev(x).requires_grad_(True)
        frozen = m.encode(xt, n)
        assert type(frozen[0].grad_fn).__name__.startswith("_EncodeGrad")
        _loss(frozen, {k: w for k, w in cot.items() if k != "cb"}).backward()
        assert all(torch.equal(a.detach(), b) for a, b in zip(frozen, out)) and torch.equal(xt.grad, dx), "d_audio differs from the audio-only backward's"
        assert all(p.grad is None for p in m.parameters())
    finally:
        m.set_precision("fp32")


def test_a_clip_does_not_depend_on_its_batch_neighbours():
    """Without a cotangent on the two losses the batch's gradient is the sum of the single-clip calls' up to summation order: the sum of the
    device's single-clip gradients is held to the batch's float64 truth by the same rule as the batch itself."""
    name, B, L, n = "dac_syn", 3, 28, 4
    x, cot = qu.inputs(name, B, L, n)
    cot = {k: cot[k] for k in ("z", "latents")}
    m = _model(name)
    out, _, _ = _run(m, x, cot, n)
    total = None
    for b in range(B):
        ob, _, gb = _run(m, x[b:b + 1], {k: w[b:b + 1] for k, w in cot.items()}, n)
        assert all(torch.equal(ob[i][0], out[i][b]) for i in range(3)), "a clip encodes differently alone"
        total = {k: v.clone() for k, v in gb.items()} if total is None else {k: total[k] + gb[k] for k in total}
    codes = out[1].cpu().numpy()
    g64 = qu.oracle(name, x, cot, n, codes=codes)
    eager = qu.oracle(name, x, cot, n, torch.float32, codes=codes)
    keep = [k for k, v in g64.items() if v is not None]         # no codebook-loss cotangent: the codebooks are off the graph, and exactly zero here
    assert all(not total[k].any() for k in total if k not in keep) and all(qu.kind(k) == "codebook" for k in total if k not in keep)
    qu.check_rule(qu.errors(_np(total), g64), qu.errors(eager, g64), f"{name} sum of {B} single-clip calls")


def test_selective_gradients_and_the_switch():
    name, B, L, n = "dac_syn", 3, 28, 4
    x, cot = qu.inputs(name, B, L, n)
    m = _fresh(name).set_encode_trainable("both")
    _, dx, full = _run(m, x, cot, n)
    full = {k: v.clone() for k, v in full.items()}
    enc = [k for k in full if k.startswith("encoder.")]
    qnt = [k for k in full if k.startswith("quantizer.")]
    alphas = [k for k in full if qu.kind(k) == "alpha"]
    for part, want in (("encoder", enc), ("quantizer", qnt), ("both", alphas)):
        m.set_encode_trainable(part)
        # everything requires a gradient for the first two: the part that was not chosen is never written
        _, dx_s, got = _run(m, x, cot, n, x_grad=part != "both", want=None if part != "both" else want)
        assert list(got) == want, "not exactly the selected parameters got a gradient"
        assert all(torch.equal(got[k], full[k]) for k in want)
        assert (dx_s is None) == (part == "both") and (dx_s is None or torch.equal(dx_s, dx))
    # the switch off: today's behaviour, no p.grad whatever requires_grad says
    m.set_encode_trainable(None)
    for p in m.parameters():
        p.requires_grad_(True)
        p.grad = None
    xt = _dev(x).requires_grad_(True)
    out = m.encode(xt, n)
    assert type(out[0].grad_fn).__name__.startswith("_EncodeGrad") and not out[4].requires_grad
    _loss(out, {k: w for k, w in cot.items() if k != "cb"}).backward()
    assert torch.equal(xt.grad, dx) and all(p.grad is None for p in m.parameters())
    assert m.encode(_dev(x), n)[0].grad_fn is None


def test_three_optimiser_steps():
    name, B, L, n = "dac_syn", 3, 28, 4
    x, cot = qu.inputs(name, B, L, n)
    m = _fresh(name).set_encode_trainable("both")
    named = _encode_named(m)
    for k, p in m.named_parameters():
        p.requires_grad_(k in named)
    opt = torch.optim.SGD(list(m.encoder_parameters()) + list(m.quantizer_parameters()), lr=0.01)
    xd = _dev(x)
    for step in range(3):
        opt.zero_grad(set_to_none=True)
        out = m.encode(xd, n)
        _loss(out, cot).backward()
        if step == 1:                                           # the gradients after one step: the re-pack and the refreshed transposed images
            sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
            codes = out[1].cpu().numpy()
            g64 = qu.oracle(name, x, cot, n, codes=codes, sd=sd)
            eager = qu.oracle(name, x, cot, n, torch.float32, codes=codes, sd=sd)
            qu.check_rule(qu.errors(_np({k: p.grad for k, p in named.items()}), g64), qu.errors(eager, g64), f"{name} after one SGD step")
        before = {k: p.detach().clone() for k, p in named.items()}
        opt.step()
        assert all(not torch.equal(before[k], p) for k, p in named.items()), "an encoder or quantiser parameter did not move"
        with torch.no_grad():
            stepped = m.encode(xd, n)
        twin = _fresh(name, {k: v.detach().cpu().clone() for k, v in m.state_dict().items()})
        with torch.no_grad():
            assert all(torch.equal(a, b) for a, b in zip(stepped, twin.encode(xd, n))), f"step {step}: the stepped model encodes differently from its twin"


def test_python_errors_of_the_parameter_path():
    name, B, L, n = "dac_syn", 3, 28, 4
    x, cot = qu.inputs(name, B, L, n)
    m = _fresh(name).set_encode_trainable("both")
    for p in m.parameters():
        p.requires_grad_(True)
    xd = _dev(x)
    # per-clip lengths, the sweep and the chunked path have no parameter gradients: refused with the switch on, served under no_grad
    with pytest.raises(NotImplementedError):
        m.encode(xd, n, lengths=[28, 20, 9])
    with pytest.raises(NotImplementedError):
        m(xd, lengths=[28, 20, 9])
    with pytest.raises(NotImplementedError):
        m.encode_sweep(xd, [1, 4])
    with pytest.raises(NotImplementedError):
        m.compress(xd[0])
    with torch.no_grad():
        assert m.encode_sweep(xd, [1, 4])[0].shape[0] == 2 and m.encode(xd, n, lengths=[28, 20, 9])[0].grad_fn is None
        assert m.compress(xd[0]).codes is not None
    # padding off: refused on the new path only
    m.padding = False
    try:
        Lp = next(t for t in range(64, 20000) if m.num_frames(t) >= 1)
        xl = torch.zeros(1, 1, Lp, device="cuda")
        with torch.no_grad():
            assert m.encode(xl)[0].grad_fn is None
        with pytest.raises(NotImplementedError):
            m.encode(xl)
    finally:
        m.padding = True
    # an in-place parameter edit between forward and backward
    out = m.encode(xd, n)
    with torch.no_grad():
        m.get_parameter("encoder.block.1.block.0.block.0.alpha").add_(0.25)
    with pytest.raises(RuntimeError, match="changed in place"):
        _loss(out, cot).backward()
    assert all(p.grad is None for p in m.parameters())
    # double backward
    p0 = m.get_parameter("encoder.block.0.bias")
    (g,) = torch.autograd.grad(_loss(m.encode(xd, n), cot), p0, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()
    # training mode refuses before anything else
    m.train()
    with pytest.raises(NotImplementedError):
        m.encode(xd, n)
    m.eval()


def test_c_level_errors_leave_the_handle_and_the_other_slots_alone():
    from esc import _native
    name, B, L, n = "dac_syn", 3, 28, 4
    x, cot = qu.inputs(name, B, L, n)
    m = _fresh(name).set_encode_trainable("both")
    xd = _dev(x).contiguous()
    with torch.no_grad():
        before = m.encode(xd, n)
    _, want_dx, want = _run(m, x, cot, n)
    lib, hd, flat, dev, st = m._ctx(xd, "x")
    P = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    v = m._version()
    T = before[0].shape[-1]
    floats = lib.escx_dac_encode_tape_floats(hd, B, L, n)
    tape = torch.empty(floats, device="cuda")
    z, codes, lat, losses = torch.empty_like(before[0]), torch.empty_like(before[1]), torch.empty_like(before[2]), torch.empty(2, device="cuda")
    _native.check(lib.escx_dac_encode_tape(hd, P(flat), v, P(xd), B, L, n, None, P(z), P(codes), P(lat), P(losses), P(tape), floats, st))
    layout = m._flat[dev.index if dev.index is not None else torch.cuda.current_device()]["layout"]
    enc_end = max(off + cnt for k, off, cnt in layout if k.startswith("encoder."))
    qnt_end = max(off + cnt for k, off, cnt in layout if k.startswith("quantizer."))
    assert min(off for k, off, cnt in layout if k.startswith("quantizer.")) == enc_end and min(off for k, off, cnt in layout if k.startswith("decoder.")) == qnt_end
    cz, cl, cm, cb = _dev(cot["z"]).contiguous(), _dev(cot["latents"]).contiguous(), _dev(cot["cm"]).reshape(1), _dev(cot["cb"]).reshape(1)
    grad, dx = torch.full_like(flat, 7.0), torch.full((B, 1, L), 7.0, device="cuda")

    def call(ver=v, tp=tape, fl=floats, audio=P(xd), gg=P(grad), parts=3, dxp=P(dx)):
        return lib.escx_dac_encode_backward_params(hd, P(flat), ver, P(tp), fl, audio, P(cz), P(cl), P(cm), P(cb), B, L, parts, dxp, gg, st)

    rc = call(ver=v + 1)                                                                                        # a stale parameter version
    assert rc == -4 and b"version" in lib.escx_last_error() and str(v).encode() in lib.escx_last_error() and str(v + 1).encode() in lib.escx_last_error()
    assert call(tp=torch.zeros(floats, device="cuda")) == -1                                                    # not a tape
    assert call(fl=floats - 64) == -1                                                                           # the wrong size
    assert call(gg=None) == -1 and call(audio=None) == -1                                                       # NULL grad_flat, NULL audio
    assert call(parts=0) == -1 and call(parts=4) == -1 and call(parts=-1) == -1
    _native.check(lib.escx_dac_set_padding(hd, 0))
    try:
        assert call() == -2
    finally:
        _native.check(lib.escx_dac_set_padding(hd, 1))
    torch.cuda.synchronize()
    assert bool((grad == 7.0).all()) and bool((dx == 7.0).all()), "a refused backward wrote an output"
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(m.encode(xd, n), before)), "the handle encodes differently after the refused calls"
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((grad[qnt_end:] == 7.0).all()), "a float outside the encoder's and the quantiser's slots was written"
    assert torch.equal(dx, want_dx)
    for k, off, cnt in layout:
        if not k.startswith("decoder."):
            assert torch.equal(grad[off:off + cnt], want[k].reshape(-1)), k
    # one part at a time, and without d_audio: the same gradients, the other part's slots untouched
    g1, g2 = torch.full_like(flat, 7.0), torch.full_like(flat, 7.0)
    assert call(gg=P(g1), parts=1, dxp=None) == 0 and call(gg=P(g2), parts=2, dxp=None) == 0
    torch.cuda.synchronize()
    assert torch.equal(g1[:enc_end], grad[:enc_end]) and bool((g1[enc_end:] == 7.0).all())
    assert torch.equal(g2[enc_end:qnt_end], grad[enc_end:qnt_end]) and bool((g2[:enc_end] == 7.0).all()) and bool((g2[qnt_end:] == 7.0).all())
    # every cotangent NULL: zeros in every chosen slot, nothing else
    g0 = torch.full_like(flat, 7.0)
    assert lib.escx_dac_encode_backward_params(hd, P(flat), v, P(tape), floats, P(xd), None, None, None, None, B, L, 3, None, P(g0), st) == 0
    torch.cuda.synchronize()
    assert bool((g0[:qnt_end] == 0).all()) and bool((g0[qnt_end:] == 7.0).all())
    # a tape of fewer stages: the later stages' slots are written as zeros
    f2 = lib.escx_dac_encode_tape_floats(hd, B, L, 2)
    tape2, c2, l2 = torch.empty(f2, device="cuda"), torch.empty(B, 2, T, dtype=torch.int64, device="cuda"), torch.empty(B, 2 * m.codebook_dim, T, device="cuda")
    _native.check(lib.escx_dac_encode_tape(hd, P(flat), v, P(xd), B, L, 2, None, P(z), P(c2), P(l2), P(losses), P(tape2), f2, st))
    g3 = torch.full_like(flat, 7.0)
    assert lib.escx_dac_encode_backward_params(hd, P(flat), v, P(tape2), f2, P(xd), P(cz), None, P(cm), P(cb), B, L, 2, None, P(g3), st) == 0
    torch.cuda.synchronize()
    late = min(off for k, off, cnt in layout if k.startswith("quantizer.quantizers.2."))
    assert bool((g3[late:qnt_end] == 0).all()) and bool(g3[enc_end:late].ne(0).any()) and bool((g3[:enc_end] == 7.0).all()) and bool((g3[qnt_end:] == 7.0).all())
