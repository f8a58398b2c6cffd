"""Mixed-length batches of the DAC baseline (esc.baselines.DAC: `lengths` in encode / forward, `frame_lengths` in decode / quantizer.from_codes;
include/escx.h escx_dac_encode_lengths, escx_dac_from_codes_lengths, escx_dac_decode_lengths): what can be checked without a device - the
validation of the per-clip lengths (before the device check, with the helper of the per-clip codebook counts), the two length helpers, the
refusals and the three symbols."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden


def _model(name="dac_syn"):
    from esc.baselines import DAC
    return DAC(**json.loads(str(load_golden(name)["config_json"]))).eval()


def _calls(m, B=3, L=64):
    """name -> (callable taking the per-clip lengths, the largest valid entry)"""
    x = torch.zeros(B, 1, L)
    T = m.num_frames(L)
    z = torch.zeros(B, m.latent_dim, T)
    codes = torch.zeros(B, m.n_codebooks, T, dtype=torch.int64)
    return {"encode": (lambda v: m.encode(x, None, lengths=v), L),
            "encode+counts": (lambda v: m.encode(x, [1, 2, 3], lengths=v), L),
            "forward": (lambda v: m(x, None, None, lengths=v), L),
            "decode": (lambda v: m.decode(z, frame_lengths=v), T),
            "from_codes": (lambda v: m.quantizer.from_codes(codes, frame_lengths=v), T),
            "from_codes+counts": (lambda v: m.quantizer.from_codes(codes, [1, 2, 3], frame_lengths=v), T)}


CALLS = ("encode", "encode+counts", "forward", "decode", "from_codes", "from_codes+counts")


@pytest.mark.parametrize("call", CALLS)
def test_bad_lengths_are_value_errors_before_the_device_check(call):
    m = _model()
    fn, hi = _calls(m)[call]
    with pytest.raises(ValueError, match="2 entries for a batch of 3"):
        fn([hi, hi])
    with pytest.raises(ValueError, match="4 entries for a batch of 3"):
        fn(torch.tensor([hi, hi, hi, hi]))
    for bad in ([hi, 2.0, hi], [hi, True, hi], [hi, "8", hi], torch.tensor([1.0, 2.0, 3.0]), torch.tensor([True, True, False]),
                torch.tensor([[hi, hi, hi]]), torch.tensor(hi)):
        with pytest.raises((ValueError, TypeError)) as e:
            fn(bad)
        assert e.type is ValueError, (call, bad)
    for bad, clip in (([hi, 0, hi], 1), ([hi, hi, hi + 1], 2), ([-3, hi, hi], 0)):
        with pytest.raises(ValueError, match=rf"\[{clip}\]"):
            fn(bad)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("form", ("list", "tuple", "numpy", "tensor"))
def test_valid_lengths_on_a_cpu_tensor_reach_the_device_check(call, form):
    m = _model()
    fn, hi = _calls(m)[call]
    v = [hi, max(1, hi // 2), hi]
    v = {"list": v, "tuple": tuple(v), "numpy": list(np.asarray(v, np.int32)), "tensor": torch.tensor(v, dtype=torch.int32)}[form]
    with pytest.raises(RuntimeError, match="HIP device"):
        fn(v)


def test_a_clip_without_a_frame_is_named():
    m = _model("dac_tiny")                                       # hop 320: 100 samples give no frame, 321 give one
    x = torch.zeros(2, 1, 640)
    assert m.num_frames(100) == 0 and m.num_frames(321) == 1
    with pytest.raises(ValueError, match="clip 1"):
        m.encode(x, lengths=[640, 100])
    with pytest.raises(RuntimeError, match="HIP device"):
        m(x, lengths=[640, 100])                                 # forward pads every clip to a multiple of the hop first: one frame
    with pytest.raises(RuntimeError, match="HIP device"):
        m.encode(x, lengths=[640, 321])


def test_length_helpers():
    for name in ("dac_syn", "dac_tiny"):
        m = _model(name)
        hop = m.hop_length
        lens = [hop, hop + 1, 2 * hop - 1, 7 * hop, 4800, 4801]
        fl = m.frame_lengths(lens)
        assert fl.dtype == torch.int64 and fl.device.type == "cpu" and fl.dim() == 1
        assert fl.tolist() == [m.num_frames(v) for v in lens]
        assert torch.equal(m.frame_lengths(torch.tensor(lens)), fl) and torch.equal(m.frame_lengths(tuple(lens)), fl)
        ol = m.output_lengths(fl)
        assert ol.dtype == torch.int64 and ol.device.type == "cpu" and ol.dim() == 1
        assert ol.tolist() == [m.output_samples(int(t)) for t in fl]
        assert fl[0] == 1 and fl[3] == 7                         # a multiple of the hop gives that many frames
        for bad in ([hop, 1.5], torch.tensor([[hop]]), [True]):
            with pytest.raises(ValueError):
                m.frame_lengths(bad)
            with pytest.raises(ValueError):
                m.output_lengths(bad)


def test_refusals():
    m = _model()
    B, L = 2, 64
    x = torch.zeros(B, 1, L)
    T = m.num_frames(L)
    z = torch.zeros(B, m.latent_dim, T)
    codes = torch.zeros(B, m.n_codebooks, T, dtype=torch.int64)
    lens, fl = [L, L // 2], [T, T // 2]
    # padding off
    m.padding = False
    for fn in (lambda: m.encode(x, lengths=lens), lambda: m(x, lengths=lens), lambda: m.decode(z, frame_lengths=fl),
               lambda: m.quantizer.from_codes(codes, frame_lengths=fl)):
        with pytest.raises(NotImplementedError, match="padding"):
            fn()
    m.padding = True
    # the sweep and the chunked file path
    with pytest.raises(NotImplementedError, match="encode_sweep"):
        m.encode_sweep(x, [1, 2], lengths=lens)
    with pytest.raises(NotImplementedError, match="compress"):
        m.compress(x, lengths=lens)
    # gradient paths: an input that requires grad ...
    xg, zg = x.clone().requires_grad_(True), z.clone().requires_grad_(True)
    for fn in (lambda: m.encode(xg, lengths=lens), lambda: m(xg, lengths=lens), lambda: m.decode(zg, frame_lengths=fl)):
        with pytest.raises(NotImplementedError, match="gradient"):
            fn()
        with torch.no_grad(), pytest.raises(RuntimeError, match="HIP device"):
            fn()                                                 # with gradients disabled it is the plain call
    # ... or a decoder that trains
    for p in m.parameters():
        p.requires_grad_(False)
    m.set_trainable("decoder")
    with pytest.raises(RuntimeError, match="HIP device"):
        m.decode(z, frame_lengths=fl)                            # no parameter requires grad: nothing to refuse
    next(m.decoder_parameters()).requires_grad_(True)
    for fn in (lambda: m.decode(z, frame_lengths=fl), lambda: m(x, lengths=lens)):
        with pytest.raises(NotImplementedError, match="gradient"):
            fn()
    with pytest.raises(RuntimeError, match="HIP device"):
        m.encode(x, lengths=lens)                                # encode has no parameter gradients: not a gradient path
    m.set_trainable(None)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.decode(z, frame_lengths=fl)


def test_calls_without_the_keyword_keep_their_signature():
    import inspect
    from esc.baselines import DAC
    for fn, kw in ((DAC.encode, "lengths"), (DAC.forward, "lengths"), (DAC.decode, "frame_lengths"), (DAC._from_codes, "frame_lengths"),
                   (DAC.encode_sweep, "lengths"), (DAC.compress, "lengths")):
        ps = list(inspect.signature(fn).parameters.values())
        assert ps[-1].name == kw and ps[-1].default is None, fn     # the new keyword comes last and defaults to today's call


def test_symbols_are_declared_and_exported():
    from esc import _native
    lib = _native.load()
    header = open(os.path.join(ROOT, "include", "escx.h")).read()
    p, i32 = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32)
    want = {"escx_dac_encode_lengths": [p, p, ctypes.c_int64, p, ctypes.c_int, ctypes.c_int, i32, ctypes.c_int, ctypes.c_int, i32, p, p, p, p, p],
            "escx_dac_from_codes_lengths": [p, p, ctypes.c_int64, p, ctypes.c_int, ctypes.c_int, ctypes.c_int, i32, i32, p, p, p],
            "escx_dac_decode_lengths": [p, p, ctypes.c_int64, p, ctypes.c_int, ctypes.c_int, i32, i32, p, p]}
    for sym, args in want.items():
        assert f"int {sym}(" in header, sym
        assert sym in _native.SIGNATURES and hasattr(lib, sym), sym
        assert _native.SIGNATURES[sym][0] is ctypes.c_int and list(_native.SIGNATURES[sym][1]) == args, sym
    # a null handle is refused without a device
    bad = _native.ESCX_ERR_INVALID_ARG
    one = (ctypes.c_int32 * 1)(4)
    assert lib.escx_dac_encode_lengths(None, None, 0, None, 1, 4, one, 1, 1, None, None, None, None, None, None) == bad
    assert lib.escx_dac_from_codes_lengths(None, None, 0, None, 1, 1, 1, one, None, None, None, None) == bad
    assert lib.escx_dac_decode_lengths(None, None, 0, None, 1, 1, one, None, None, None) == bad
