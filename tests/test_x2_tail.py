"""The two-term (f16x2) PatchSplit epilogue of the split-operand MLP (fused_mlp_x3.h SPLIT, NT = 2): two fp16 terms per operand under the range rule's power-of-two
scales, three cross products per full K step and the PAIRED last step where C / 16 is odd (C = 72 -> 80 and C = 144: one fragment [w_hi | w_lo] against
[y_hi | y_hi] and [y_lo | 0], two matrix steps where the zero-padded step took three).

Every case drives escx_transformer_layer as tests/test_attn_stream.py does, with the project's own bounds: ACT_TOL against the float32 oracle, and device error
<= 1.1 x the oracle's float32 error + 1e-7 against its float64 evaluation.

Which launch a decoder layer's last MLP takes depends on the clip's geometry alone: up to 1200 tokens per clip it is the hidden-split form (raw partial sums, a
combine launch, PatchSplit as its own launch), above that the one-launch form with PatchSplit in its epilogue.  The narrow maps (W = 6, W = 22) therefore cover the
plain MLP, the attention and the stand-alone PatchSplit at the tail widths, and the WIDE cases below are the ones that reach the epilogue - they assert that the
mlp_x3_split launch was taken, so a changed threshold cannot silently empty them."""
import ctypes
import json

import pytest
import torch

from gpu_util import build_models, rel_rms
from esc import _native
from test_gpu_parity import ACT_TOL, _h, _layer_cases, _ptr

pytestmark = pytest.mark.gpu

TAIL_WIDTHS = (45, 72, 144)         # padded 48, 80, 144: C / 16 odd, the last 32-deep K step is half empty
CONTROL = 96                        # no tail
# decoder layers whose PatchSplit runs in the MLP epilogue, at the smallest maps above 1200 tokens per clip (W is a multiple of the quantiser overlap, 2, and
# W % 4 = 2 adds padded window slots): C = 144 (H = 8) 1232 tokens = 77 row tiles, C = 96 (H = 16) 1248 tokens = 78 tiles, C = 72 (H = 32) 1216 tokens = 76 tiles.
# 77 and 78 tiles leave the last workgroup (4 or 8 waves) partial; H >= 8 and an even W make the tokens a multiple of 16, so no row tile of these layers is partial:
# the dead rows the kernel must keep out are the whole tiles of the idle waves of that last workgroup.
WIDE = {144: 154, 96: 78, 72: 38}


def _run_layer(lib, hd, lid, x, B, H, W, out_shape):
    y = torch.empty(out_shape, device="cuda")
    Hn = ctypes.c_int()
    xg = x.cuda()
    _native.check(lib.escx_transformer_layer(hd, lid, _ptr(xg), B, H, W, _ptr(y), ctypes.byref(Hn), None))
    return y.cpu(), Hn.value


def _launches(lib, hd, lid, x, B, H, W, out_shape):
    """names of the launch groups one layer call takes"""
    lib.escx_profile_enable(hd, 2)
    _run_layer(lib, hd, lid, x, B, H, W, out_shape)
    recs = json.loads(lib.escx_profile_report(hd).decode())
    lib.escx_profile_enable(hd, 0)
    return {r["name"].split("[")[0] for r in recs}


_MODELS = {}


def _models(name):
    if name not in _MODELS:
        _MODELS[name] = build_models(name, "f16x2")
    return _MODELS[name]


_REF = {}


def _refs(name, lid, B, W, seed, edit_key=None, orc=None, cfg=None):
    """(x, float32 oracle output, float64 oracle output, H') of one layer on one input - computed once, shared by the tests, never modified."""
    key = (name, lid, B, W, seed, edit_key)
    if key not in _REF:
        from oracle import esc_oracle as O
        if orc is None:
            _, orc, _, cfg = _models(name)
        case = [c for c in _layer_cases(cfg) if c[0] == lid][0]
        _, pfx, C, nH, scale, H = case
        sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in orc.sd.items()}
        x = torch.randn(B, H * W, C, generator=torch.Generator().manual_seed(seed + 131 * lid))
        ref32, Hr, _ = O.transformer_layer(x, H, W, orc.sd, pfx, nH, cfg["swin_depth"], cfg["window_size"], scale)
        ref64, _, _ = O.transformer_layer(x.double(), H, W, sd64, pfx, nH, cfg["swin_depth"], cfg["window_size"], scale)
        _REF[key] = (x, ref32, ref64, Hr)
    return _REF[key]


def _check_fp64(name, lid, B, W, seed, tag):
    model, orc, g, cfg = _models(name)
    lib, hd = _h(model)
    assert model.precision == "f16x2"
    case = [c for c in _layer_cases(cfg) if c[0] == lid][0]
    _, pfx, C, nH, scale, H = case
    x, ref32, ref64, Hr = _refs(name, lid, B, W, seed)
    y, Hn = _run_layer(lib, hd, lid, x, B, H, W, ref32.shape)
    assert Hn == Hr
    assert torch.isfinite(y).all()
    e_dev, e_cpu = rel_rms(y.double(), ref64), rel_rms(ref32.double(), ref64)
    print(f"[{tag} B={B} W={W}] layer {lid:2d} {pfx:22s} C={C:3d}: device {e_dev:.2e}   reference float32 {e_cpu:.2e}   ratio {e_dev / max(e_cpu, 1e-30):.2f}")
    assert e_dev <= 1.1 * e_cpu + 1e-7, f"{name} layer {lid} ({pfx}) B={B} W={W}: device error {e_dev:.3e} vs float32 reference error {e_cpu:.3e}"


@pytest.mark.parametrize("B,W", [(1, 6), (3, 22)])
def test_tail_widths_against_fp64(B, W):
    """ESC-Base, f16x2: every layer with C in {45, 72, 144} and C = 96 as the no-tail control, encoder and decoder; at B = 1, W = 6 and B = 3, W = 22 the last wave and
    the last workgroup are partial.  Against float64 with the 1.1 x bound."""
    _, _, _, cfg = _models("base")
    n = 0
    for lid, pfx, C, nH, scale, H in _layer_cases(cfg):
        if C in TAIL_WIDTHS or C == CONTROL:
            _check_fp64("base", lid, B, W, 43, "x2 tail")
            n += 1
    assert n == 9               # pre_nn, encoder.blocks.0-3, decoder.blocks.2-4, post_nn: every layer but the C = 192 / 384 ones


@pytest.mark.parametrize("C", [144, 96, 72])
def test_split_epilogue_against_fp64(C):
    """The decoder layers at C = 144 / 96 / 72 on maps wide enough for the one-launch MLP: the two-term PatchSplit epilogue (paired tail at 144 and 72, none at 96)
    against float64 with the 1.1 x bound; the launch under test is asserted to be the one taken."""
    model, _, _, cfg = _models("base")
    lib, hd = _h(model)
    lid, pfx, _, nH, scale, H = [c for c in _layer_cases(cfg) if c[2] == C and c[4] == "up"][0]
    W = WIDE[C]
    x, ref32, _, _ = _refs("base", lid, 1, W, 47)
    names = _launches(lib, hd, lid, x, 1, H, W, ref32.shape)
    assert "mlp_x3_split" in names and "split_fused" not in names, names
    _check_fp64("base", lid, 1, W, 47, "x2 epilogue")


def _lopsided(sd):
    """PatchSplit norms and weights moved apart by powers of two (exact in fp32, so the oracle's output only changes scale): the activation scale sy and the weight scale
    2^k of the epilogue's range rule then differ by up to 2^26, and at C = 72 the norm's BETA, not its gamma, decides the bound."""
    n = 0
    for j, (gn, bn, wn) in {2: (2.0 ** 14, 2.0 ** 14, 2.0 ** -12), 3: (2.0 ** -10, 2.0 ** -10, 2.0 ** 9), 4: (1.0, 2.0 ** 8, 2.0 ** -3)}.items():
        p = f"decoder.blocks.{j}.subsample."
        sd[p + "norm.weight"] = sd[p + "norm.weight"] * gn
        sd[p + "norm.bias"] = sd[p + "norm.bias"] * bn
        sd[p + "up.weight"] = sd[p + "up.weight"] * wn
        n += 1
    assert n == 3


def test_range_rule_of_the_two_term_epilogue():
    """A model whose PatchSplit norms and weights are lopsided by powers of two (as tests/test_scale_fold.py builds its lopsided MLP): unscaled, the 2^14 norm output
    would overflow fp16's high term and the 2^-12 / 2^-10 operands would lose their low terms to subnormals.  Against the float32 oracle within ACT_TOL, output finite."""
    model, orc, g, cfg = build_models("base", "f16x2", _lopsided)
    lib, hd = _h(model)
    for C in (144, 96, 72):
        lid, pfx, _, nH, scale, H = [c for c in _layer_cases(cfg) if c[2] == C and c[4] == "up"][0]
        W = WIDE[C]
        x, ref32, _, Hr = _refs("base", lid, 1, W, 53, "lopsided", orc, cfg)
        names = _launches(lib, hd, lid, x, 1, H, W, ref32.shape)
        assert "mlp_x3_split" in names, names
        y, Hn = _run_layer(lib, hd, lid, x, 1, H, W, ref32.shape)
        assert Hn == Hr
        assert torch.isfinite(y).all()
        err = rel_rms(y, ref32)
        print(f"[x2 epilogue range] layer {lid} C={C}: rel rms {err:.3e}, output rms {float(ref32.double().pow(2).mean().sqrt()):.3e}")
        assert err < ACT_TOL, f"layer {lid} ({pfx}): rel rms {err:.3e}"


def test_precision_round_trip_repacks_the_epilogue_image():
    """f16x2 -> bf16x3 -> f16x2 on one handle over the epilogue layers (wide maps) and the tail-width layers (W = 22): the three-term image overwrites the whole
    allocation, so the first and third outputs are bit-identical only if the two-term image and its trailer are re-packed in place; the middle one within ACT_TOL."""
    model, orc, g, cfg = build_models("base", "f16x2")
    lib, hd = _h(model)
    runs = []
    for lid, pfx, C, nH, scale, H in _layer_cases(cfg):
        if C in TAIL_WIDTHS or C == CONTROL:
            runs.append((lid, H, 3, 22, 43))
            if scale == "up":
                runs.append((lid, H, 1, WIDE[C], 47))

    def sweep():
        out = {}
        for lid, H, B, W, seed in runs:
            x, ref32, _, _ = _refs("base", lid, B, W, seed)
            out[lid, W] = _run_layer(lib, hd, lid, x, B, H, W, ref32.shape)[0]
        return out

    first = sweep()
    model.set_precision("bf16x3")
    second = sweep()
    model.set_precision("f16x2")
    third = sweep()
    assert len(first) == 12                 # nine layers at W = 22, the three epilogue layers on their wide maps
    for (lid, H, B, W, seed) in runs:
        ref32 = _refs("base", lid, B, W, seed)[1]
        assert torch.isfinite(first[lid, W]).all()
        assert torch.equal(first[lid, W], third[lid, W]), f"layer {lid} W={W}: f16x2 output changed after a round trip through bf16x3"
        assert rel_rms(second[lid, W], ref32) < ACT_TOL, f"layer {lid} W={W}: bf16x3 rel rms {rel_rms(second[lid, W], ref32):.3e}"
        assert not torch.equal(first[lid, W], second[lid, W])           # the modes really are different arithmetic


def test_same_launch_twice_is_bit_identical():
    """C = 45, the C = 72 decoder layer (narrow map and the epilogue's wide one) and the C = 144 encoder layer: two calls on the same input give the same bits."""
    model, _, _, cfg = _models("base")
    lib, hd = _h(model)
    cases = _layer_cases(cfg)
    pick = [(c, 3, 22, 43) for c in cases if c[2] == 45 or (c[2] == 72 and c[4] == "up") or (c[2] == 144 and c[4] == "down")]
    pick.append(([c for c in cases if c[2] == 72 and c[4] == "up"][0], 1, WIDE[72], 47))
    assert len(pick) == 6
    for (lid, pfx, C, nH, scale, H), B, W, seed in pick:
        x, ref32, _, _ = _refs("base", lid, B, W, seed)
        a = _run_layer(lib, hd, lid, x, B, H, W, ref32.shape)[0]
        b = _run_layer(lib, hd, lid, x, B, H, W, ref32.shape)[0]
        assert torch.equal(a, b), f"layer {lid} ({pfx}) W={W}: two launches differ"


def test_large_tail_widths_against_fp64():
    """ESC-Large (other head mappings at the tail widths), f16x2, B = 1, W = 6: every layer against float64."""
    _, _, _, cfg = _models("large")
    for lid, pfx, C, nH, scale, H in _layer_cases(cfg):
        _check_fp64("large", lid, 1, 6, 59, "x2 tail large")
