"""The two-term (f16x2) split-operand MLP reads its fc1 bias and its LayerNorm gamma / beta PRE-SCALED from the packed weight image (fused_mlp_x3.h): the power-of-two
factors 2^k1, sx, sh of the range rule are applied when the image is packed, not per token.  With the default synthetic weights a wrong factor could hide behind scales that
happen to agree, so these tests run a small codec whose MLPs have deliberately lopsided scales:

  * geometry: the smallest one the fused mlp_x3 path accepts - widths 45 (padded 48) and 96, 8 and 4 frequency rows.  Three clips of 120 samples (6 frames: 144 tokens
    at the 48-wide scale = full 16-row tiles, 36 tokens at the 96-wide scale = two full tiles and one of 4 rows): maps this small take the hidden-split form of the kernel
    (raw partial sums + combine launch).  Two clips of 12040 samples (602 and 301 frames: more than 1200 tokens per clip at both scales, 2408 tokens = 150.5 tiles at the
    96-wide one): the plain bias + residual epilogue and, in the decoder, the PatchSplit epilogue (mlp_x3_split);
  * weights: synthetic, then every block's fc1 weight and bias x 2^6 and fc2 weight x 2^-5 (k1 and k2 move apart, the bound of the GELU output moves with k1), and the
    fc1 bias of one block at each width x 2^4 on top (the bias term, not the row norm, then decides sh there).

Bounds: the ones tests/test_gpu_parity.py uses for the mode - every code equal to the oracle's (the clips are chosen free of reference near-ties, which
test_oracle_is_finite_and_free_of_near_ties checks without a GPU) and audio within AUDIO_TOL RMS."""
import json

import numpy as np
import pytest
import torch

from gpu_util import NEAR_TIE, code_report, rms
from esc import synth

CFG = {"backbone": "transformer", "in_dim": 2, "in_freq": 24, "h_dims": [45, 96], "max_streams": 2, "win_len": 2.5, "hop_len": 0.625, "sr": 16000, "patch_size": [3, 2],
       "swin_heads": [3], "swin_depth": 2, "window_size": 4, "mlp_ratio": 4.0, "overlap": 2, "group_size": 3, "codebook_size": 64, "codebook_dims": [4, 4], "l2norm": True}
LENGTHS = (120, 12040)
FAMILIES = {120: {"mlp_x3", "mlp_combine"}, 12040: {"mlp_x3", "mlp_x3_split"}}       # launch families of the MLPs per clip length (hidden split below 1200 tokens per clip)
BIG_BIAS = ("encoder.pre_nn.swint_blocks.0.mlp.linear_1.bias", "decoder.blocks.0.swint_blocks.1.mlp.linear_1.bias")        # one block at 48, one at 96
MARGIN_FLOOR = 10 * NEAR_TIE        # NEAR_TIE is the gap below which the suite accepts an argmin flip as fp32 re-association noise; the clips keep every reference margin ten times above it, so no code may differ


def _state():
    from esc.models.codecs import state_manifest
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.synth_state_dict({k: list(v) for k, v in state_manifest(CFG).items()}).items()}
    n = 0
    for k in sd:
        if k.endswith(".window"):
            sd[k] = torch.hann_window(sd[k].shape[0])
        elif k.endswith("mlp.linear_1.weight") or k.endswith("mlp.linear_1.bias"):
            sd[k] = sd[k] * 2.0 ** 6; n += 1
        elif k.endswith("mlp.linear_2.weight"):
            sd[k] = sd[k] * 2.0 ** -5; n += 1
    assert n == 3 * 8, n                # pre_nn, one encoder stage, one decoder stage, post_nn: two blocks each
    for k in BIG_BIAS:
        sd[k] = sd[k] * 2.0 ** 4
    return sd


def _clips(L):
    pcm = [synth.noise_clip_int16(f"scale-fold-{L}-0", L), synth.voiced_clip_int16(f"scale-fold-{L}-1", L)]
    if L < 1000:
        pcm.append(synth.noise_clip_int16(f"scale-fold-{L}-2", L, amp=0.3))
    pcm = np.stack(pcm)
    return torch.from_numpy(synth.pcm_to_float(pcm))


_ORACLE = {}


def _oracle():
    """(oracle, {L: (clips, codes, shape, margins, audio)}) - computed once per session."""
    if not _ORACLE:
        from oracle.esc_oracle import EscOracle, Trace
        orc = EscOracle(CFG, _state())
        ref = {}
        for L in LENGTHS:
            x = _clips(L)
            tr = Trace()
            codes, shape = orc.encode(x, CFG["max_streams"], trace=tr)
            ref[L] = (x, codes.numpy(), shape, torch.stack(tr.margins, dim=1).numpy(), orc.decode(codes, shape).numpy())
        _ORACLE["v"] = (orc, ref)
    return _ORACLE["v"]


def test_oracle_is_finite_and_free_of_near_ties():
    """Without a GPU: the rescaled weights leave the oracle finite, and no reference argmin of the chosen clips sits near a tie - the GPU tests may then demand equal codes."""
    _, ref = _oracle()
    for L, (x, codes, shape, margins, audio) in ref.items():
        assert np.isfinite(audio).all() and np.isfinite(margins).all()
        assert 1e-3 < float(np.sqrt(np.mean(audio.astype(np.float64) ** 2))) < 1.0           # an audible signal of ordinary scale: AUDIO_TOL applies as it stands
        assert margins.min() > MARGIN_FLOOR, f"L {L}: reference margin {margins.min():.3e}"
        assert len(np.unique(codes)) > 8                                                      # not a collapsed quantiser


@pytest.fixture(scope="module")
def model():
    from esc.models import make_model
    m = make_model(CFG)
    m.load_state_dict(_state(), strict=True)
    return m.to("cuda:0").eval()


def _run(model, L):
    x, ref_codes, shape, _, _ = _oracle()[1][L]
    codes, gshape = model.encode(x.cuda(), CFG["max_streams"])
    assert tuple(gshape) == tuple(shape)
    wave = model.decode(torch.from_numpy(ref_codes).cuda(), shape)
    torch.cuda.synchronize()
    return codes.cpu().numpy(), wave.cpu().numpy()


def _mlp_launch_families(model, L):
    lib, hd = model._handle(torch.device("cuda:0"))
    x = _oracle()[1][L][0].cuda()
    lib.escx_profile_enable(hd, 2)
    c, s = model.encode(x, CFG["max_streams"]); model.decode(c, s)
    recs = json.loads(lib.escx_profile_report(hd).decode())
    lib.escx_profile_enable(hd, 0)
    return {r["name"].split("[")[0] for r in recs if "mlp" in r["name"]}


@pytest.mark.gpu
def test_two_term_mlp_with_lopsided_scales_against_the_oracle(model):
    from test_gpu_parity import AUDIO_TOL
    model.set_precision("f16x2")
    for L in LENGTHS:                       # every MLP of this geometry runs the split-operand kernel under test, in all three of its forms
        assert _mlp_launch_families(model, L) == FAMILIES[L], (L, _mlp_launch_families(model, L))
    out = {}
    for precision in ("f16x2", "bf16x3"):
        model.set_precision(precision)
        for L in LENGTHS:
            _, ref_codes, _, margins, ref_audio = _oracle()[1][L]
            codes, wave = _run(model, L)
            out[precision, L] = (codes, wave)
            print(f"[scale fold {precision} L {L}] audio rms vs oracle {rms(wave, ref_audio):.3e}, differing codes {int((codes != ref_codes).sum())}")
            assert np.isfinite(wave).all()
            assert np.array_equal(codes, ref_codes), f"{precision} L {L}: " + code_report(codes, ref_codes, margins)
            assert rms(wave, ref_audio) <= AUDIO_TOL, f"{precision} L {L}: audio rms {rms(wave, ref_audio):.3e}"
    for L in LENGTHS:
        assert np.array_equal(out["f16x2", L][0], out["bf16x3", L][0])
        assert rms(out["f16x2", L][1], out["bf16x3", L][1]) <= AUDIO_TOL


@pytest.mark.gpu
def test_prescaled_arrays_are_repacked_with_the_image(model):
    """f16x2 -> bf16x3 -> f16x2: the three-term image overwrites the buffer, so the two-term outputs are bitwise the earlier ones only if the pre-scaled bias / gamma / beta
    are written again with the fragments."""
    model.set_precision("f16x2")
    before = {L: _run(model, L) for L in LENGTHS}
    model.set_precision("bf16x3")
    other = _run(model, LENGTHS[0])
    model.set_precision("f16x2")
    for L in LENGTHS:
        codes, wave = _run(model, L)
        assert np.array_equal(codes, before[L][0])
        assert np.array_equal(wave.view(np.uint32), before[L][1].view(np.uint32)), f"L {L}: {int((wave != before[L][1]).sum())} samples differ after the round trip"
    assert not np.array_equal(other[1].view(np.uint32), before[LENGTHS[0]][1].view(np.uint32))           # the modes are different arithmetic: the round trip did re-pack
