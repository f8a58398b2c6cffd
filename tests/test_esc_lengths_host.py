"""Mixed-length batches of esc.ESC (`lengths` in encode / eval forward, `frame_lengths` in decode; include/escx.h escx_encode_lengths,
escx_decode_lengths, escx_forward_lengths): what can be checked without a device - the two length helpers, every refusal that is raised before the
device check, the three symbols, and the oracle fact that motivates the feature: zero-padding a clip changes the codes inside its own frames."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden, synth_state


def _cfg(name):
    return json.loads(str(load_golden(name)["config_json"]))


def _model(name="tiny", cls="csvq+swinT", **over):
    from esc.models import make_model
    return make_model(dict(_cfg(name), **over), cls).eval()


def _clip(L):
    from esc import synth
    return torch.from_numpy(synth.pcm_to_float(synth.voiced_clip_int16(f"len{L}", L))).reshape(-1)


@pytest.mark.parametrize("name,lengths,widths", [("tiny", [1280, 70, 490, 570, 1279], [32, 2, 12, 14, 32]),
                                                 ("base", [8000, 7680, 4080, 560, 2240], [50, 48, 26, 4, 14])])
def test_length_helpers_follow_latent_shape(name, lengths, widths):
    m = _model(name)
    assert m.frame_lengths(lengths) == widths == [m.latent_shape(L)[1] for L in lengths]
    assert m.frame_lengths(torch.tensor(lengths)) == widths
    pt = m.cfg["patch_size"][1]
    assert m.output_lengths(widths) == [m.hop_length * (pt * W - 1) for W in widths] == m.output_lengths(torch.tensor(widths))


def _calls(m, B=3, L=1280):
    x = torch.zeros(B, L)
    H, W = m.latent_shape(L)
    codes = torch.zeros(B, 3, m.cfg["group_size"], W // m.cfg["overlap"], dtype=torch.int64)
    return {"encode": (lambda v, s=3: m.encode(x, s, lengths=v), L),
            "forward": (lambda v, s=3: m(x, None, s, lengths=v), L),
            "decode": (lambda v, s=None: m.decode(codes, (H, W), num_streams=s, frame_lengths=v), W)}


CALLS = ("encode", "forward", "decode")


@pytest.mark.parametrize("call", CALLS)
def test_bad_lengths_are_value_errors_before_the_device_check(call):
    fn, hi = _calls(_model())[call]
    with pytest.raises(ValueError, match="2 entries for a batch of 3"):
        fn([hi, hi])
    with pytest.raises(ValueError, match="4 entries for a batch of 3"):
        fn(torch.tensor([hi, hi, hi, hi]))
    for bad in ([hi, 2.0, hi], [hi, True, hi], [hi, "8", hi], torch.tensor([1.0, 2.0, 3.0]), torch.tensor([True, True, False]),
                torch.tensor([[hi, hi, hi]]), torch.tensor(hi), "123", 7):
        with pytest.raises((ValueError, TypeError)) as e:
            fn(bad)
        assert e.type is ValueError, (call, bad)
    for bad, clip in (([hi, 0, hi], 1), ([hi, hi, hi + 1], 2), ([-3, hi, hi], 0)):
        with pytest.raises(ValueError, match=rf"\[{clip}\]"):
            fn(bad)


def test_a_clip_at_or_below_the_reflect_padding_is_refused():
    m = _model()
    half = m.in_freq - 1                    # n_fft // 2
    for call in ("encode", "forward"):
        fn, hi = _calls(m)[call]
        with pytest.raises(ValueError, match=r"lengths\[1\]"):
            fn([hi, half, hi])


@pytest.mark.parametrize("call", CALLS)
def test_an_odd_latent_width_is_the_single_clip_assertion_and_names_the_clip(call):
    m = _model()
    fn, hi = _calls(m)[call]
    odd = 120 if call != "decode" else 3    # 120 samples: 7 frames, 3 latent frames
    with pytest.raises(AssertionError, match="Time dimension must be multiple of overlap") as e:
        fn([hi, hi, odd])
    assert "clip 2" in str(e.value)


@pytest.mark.parametrize("call", CALLS)
@pytest.mark.parametrize("form", ("list", "tuple", "numpy", "tensor"))
def test_valid_lengths_on_a_cpu_tensor_reach_the_device_check(call, form):
    fn, hi = _calls(_model())[call]
    v = [hi, hi // 2, hi]
    v = {"list": v, "tuple": tuple(v), "numpy": np.asarray(v), "tensor": torch.tensor(v)}[form]
    with pytest.raises(RuntimeError, match="must live on a HIP device"):
        fn(v)


@pytest.mark.parametrize("call", CALLS)
def test_refusals_say_what_is_not_implemented(call):
    m = _model()
    fn, hi = _calls(m)[call]
    v = [hi, hi, hi]
    with pytest.raises(NotImplementedError, match="per-clip num_streams"):
        fn(v, [1, 2, 3])
    with pytest.raises(NotImplementedError, match="window_size 4 only"):
        _calls(_model(window_size=2))[call][0](v)
    rvq = _model("rvq_base", "rvq+swinT")
    x = torch.zeros(2, 8000)
    H, W = rvq.latent_shape(8000)
    with pytest.raises(NotImplementedError, match="RVQCodecs"):
        {"encode": lambda: rvq.encode(x, 2, lengths=[8000, 4080]),
         "forward": lambda: rvq(x, None, 2, lengths=[8000, 4080]),
         "decode": lambda: rvq.decode(torch.zeros(2, 2, rvq.cfg["group_size"], W // 2, dtype=torch.int64), (H, W), frame_lengths=[W, W])}[call]()
    m.train()
    with pytest.raises(ValueError, match="inference feature"):
        fn(v)


def test_x_feat_with_lengths_is_refused():
    m = _model()
    x = torch.zeros(2, 1280)
    with pytest.raises(NotImplementedError, match="x_feat"):
        m(x, torch.zeros(2, m.in_freq, 65, 2), 3, lengths=[1280, 570])


def test_calls_without_lengths_keep_their_signature_defaults():
    import inspect
    from esc.models import ESC, RVQCodecs
    for cls in (ESC, RVQCodecs):
        assert inspect.signature(cls.encode).parameters["lengths"].default is None
        assert inspect.signature(cls.forward).parameters["lengths"].default is None
    assert inspect.signature(ESC.decode).parameters["frame_lengths"].default is None


def test_symbols_are_declared_and_cite_the_reference():
    from esc import _native
    header = open(os.path.join(ROOT, "include", "escx.h")).read()
    for name, cite in (("escx_encode_lengths", "codecs.py:68-81"), ("escx_decode_lengths", "codecs.py:83-94"), ("escx_forward_lengths", "codecs.py:30-66")):
        assert name in _native.SIGNATURES
        at = header.index(f"int {name}(")
        assert cite in header[header.rindex("/*", 0, at):at], f"{name}: the comment above it does not cite {cite}"
    lib = _native.load()
    for name in ("escx_encode_lengths", "escx_decode_lengths", "escx_forward_lengths"):
        assert hasattr(lib, name)


@pytest.mark.parametrize("name,L,Lpad,S", [("tiny", 570, 1280, 3), ("base", 4080, 8000, 6)])
def test_zero_padding_changes_the_codes_inside_the_clips_own_frames(name, L, Lpad, S):
    """Why a mixed-length batch cannot be the zero-padded one: ESC is not local in time (reflect padding of the STFT, rolled windows, window padding and
    shift mask at the right edge, zero-padded de-embedding), so the oracle's codes of the padded clip differ from the clip's own within its own frames."""
    from oracle.esc_oracle import EscOracle
    orc = EscOracle(_cfg(name), synth_state(name))
    c = _clip(L)
    own, shape = orc.encode(c[None], S)
    padded, _ = orc.encode(torch.cat([c, torch.zeros(Lpad - L)])[None], S)
    n = int((padded[..., :own.shape[-1]] != own).sum())
    print(f"{name}: zero-padding {L} -> {Lpad} samples changes {n} of {own.numel()} codes inside the clip's own frames")
    assert n > 0
    assert n == {"tiny": 7, "base": 36}[name] and own.numel() == {"tiny": 63, "base": 234}[name]
