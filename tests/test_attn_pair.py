"""Paired head groups in the two-term (f16x2) attention: two head groups (MODE 2: the two halves of one) share the 32-deep fp16 steps of the output projection,
their tiles share one eight-tile unit of the weight stream ([Q_A K_A V_A Q_B K_B V_B P_0 P_1]).  The pairing is a rule of the layer's geometry: an even group
count pairs, an odd one keeps the single walk on the single layout.

Every case drives escx_transformer_layer like tests/test_attn_stream.py.  Tolerances are the project's own: ACT_TOL against the float32 oracle, and
device error <= 1.1 x the oracle's float32 error + 1e-7 against its float64 evaluation (test_layer_accuracy_against_fp64)."""
import json

import numpy as np
import pytest
import torch

from gpu_util import build_models, load_golden, rel_rms
from test_attn_stream import _out_shape, _run_layer
from test_gpu_parity import ACT_TOL, _h, _layer_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def base_f16x2():
    return build_models("base", "f16x2")


@pytest.fixture(scope="module")
def large_f16x2():
    model, orc, g, cfg = build_models("large", "f16x2")
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in orc.sd.items()}
    return model, orc, cfg, sd64


@pytest.mark.parametrize("B,W", [(1, 6), (3, 22)])
def test_large_every_layer_against_fp64(large_f16x2, B, W):
    """ESC-Large (depth 4), f16x2, every layer at its natural H against the oracle in float64.  W = 6: one full window column and one half-padded; B = 1 / 3 give odd
    window counts, so the last wave and the last workgroup are partial.  (Neither width is a multiple of 4, so the H = 2 scale does not take the packed
    half-window kernel here: its C = 384 layers run the float32 attn_fused_kernel<384>, which this change leaves alone.)"""
    from oracle import esc_oracle as O
    model, orc, cfg, sd64 = large_f16x2
    lib, hd = _h(model)
    assert model.precision == "f16x2"
    torch.manual_seed(43)
    for lid, pfx, C, nH, scale, H in _layer_cases(cfg):
        x = torch.randn(B, H * W, C)
        ref64, Hr, _ = O.transformer_layer(x.double(), H, W, sd64, pfx, nH, cfg["swin_depth"], cfg["window_size"], scale)
        ref32, _, _ = O.transformer_layer(x, H, W, orc.sd, pfx, nH, cfg["swin_depth"], cfg["window_size"], scale)
        y, Hn = _run_layer(lib, hd, lid, x, B, H, W, ref32.shape)
        assert Hn == Hr
        e_dev, e_cpu = rel_rms(y.double(), ref64), rel_rms(ref32.double(), ref64)
        print(f"[pair fp64 B={B} W={W}] layer {lid:2d} {pfx:22s} C={C:3d}: device {e_dev:.2e}   reference float32 {e_cpu:.2e}   ratio {e_dev / max(e_cpu, 1e-30):.2f}")
        assert e_dev <= 1.1 * e_cpu + 1e-7, f"layer {lid} ({pfx}) B={B} W={W}: device error {e_dev:.3e} vs float32 reference error {e_cpu:.3e}"


def _derived_from_base(h_dims, swin_heads):
    """(model on cuda:0 in f16x2, oracle, cfg): Base with other widths / head counts, name-keyed synthetic weights as bench.py's build_model makes them."""
    from esc import synth
    from esc.models import make_model
    from esc.models.codecs import state_manifest
    from oracle.esc_oracle import EscOracle
    cfg = json.loads(str(load_golden("base")["config_json"]))
    assert cfg["h_dims"] == [45, 72, 96, 144, 192, 384] and cfg["swin_heads"] == [3, 6, 12, 24, 24]
    cfg["h_dims"], cfg["swin_heads"] = list(h_dims), list(swin_heads)
    model = make_model(cfg)
    sd = {}
    for k, shp in state_manifest(model.cfg).items():
        v = synth.synth_tensor(k, shp)
        if k.endswith(".window"):
            v = torch.hann_window(shp[0]).numpy()
        sd[k] = torch.from_numpy(np.ascontiguousarray(v))
    model.load_state_dict(sd, strict=True)
    model = model.to("cuda:0").eval()
    model.set_precision("f16x2")
    return model, EscOracle(model.cfg, sd), model.cfg


def _check_layers_fp32(model, orc, cfg, wanted, seed, tag):
    from oracle import esc_oracle as O
    lib, hd = _h(model)
    cases = {c[1]: c for c in _layer_cases(cfg)}
    torch.manual_seed(seed)
    B, W = 2, 22
    for pfx, want in wanted:
        lid, _, C, nH, scale, H = cases[pfx]
        assert (C, nH) == want
        x = torch.randn(B, H * W, C)
        ref, Hr, _ = O.transformer_layer(x, H, W, orc.sd, pfx, nH, cfg["swin_depth"], cfg["window_size"], scale)
        y, Hn = _run_layer(lib, hd, lid, x, B, H, W, ref.shape)
        assert Hn == Hr
        err = rel_rms(y, ref)
        print(f"[{tag}] {pfx} C={C} heads={nH}: rel rms {err:.3e}")
        assert err < ACT_TOL, f"{pfx} C={C} heads={nH}: rel rms {err:.3e}"


def test_odd_group_count_keeps_the_single_walk():
    """A configuration derived from Base: the C = 144 encoder layer with 9 heads of 16 dims (one head per tile, 9 head groups: no pairing) next to the C = 72 decoder
    layer with its 3 heads of 24 dims (one head over two tiles: the halves pair, the odd group count is no obstacle).  f16x2 at B = 2, W = 22 against the float32
    oracle.  (9 heads must divide the decoder's second width as well: it is 144 here.)"""
    model, orc, cfg = _derived_from_base([45, 72, 96, 144, 144, 384], [3, 6, 12, 9, 24])
    _check_layers_fp32(model, orc, cfg, (("encoder.blocks.3.", (144, 9)), ("decoder.blocks.4.", (72, 3))), 47, "pair odd")


def test_odd_group_count_with_two_heads_per_tile():
    """18 heads of 8 dims at C = 144 (encoder and decoder): two heads per tile in 9 head groups - the single walk of that mapping, in a model whose other layers pair."""
    model, orc, cfg = _derived_from_base([45, 72, 144, 144, 144, 384], [3, 6, 18, 9, 24])
    _check_layers_fp32(model, orc, cfg, (("encoder.blocks.2.", (144, 18)), ("decoder.blocks.2.", (144, 18))), 61, "pair odd, two heads per tile")


def test_paired_and_single_walks_share_one_image(base_f16x2):
    """f16x2 -> fp32 -> f16x2 on one handle (set_precision re-packs the paired stream in place): first and third outputs bit-identical, the fp32 output within ACT_TOL
    of them.  C = 96, 144, 192 (paired, both head mappings).  C = 384 is never paired, and at W = 22 (no multiple of 4) it does not take the packed two-term
    kernel either: it runs the float32 attn_fused_kernel<384> in both precisions, so for it the case only shows that the re-pack of its image disturbs nothing.
    The packed two-term kernel at W % 4 == 0 is covered by tests/test_attn_stream.py and the parity tests; its stream keeps the single layout."""
    model, orc, g, cfg = base_f16x2
    lib, hd = _h(model)
    cases = [c for c in _layer_cases(cfg) if c[2] in (96, 144, 192, 384)]
    assert sorted({c[2] for c in cases}) == [96, 144, 192, 384]
    torch.manual_seed(53)
    W, B = 22, 3
    xs = {lid: torch.randn(B, H * W, C) for lid, pfx, C, nH, scale, H in cases}

    def sweep():
        return {lid: _run_layer(lib, hd, lid, xs[lid], B, H, W, _out_shape(B, H, W, C, scale, cfg, lid))[0] for lid, pfx, C, nH, scale, H in cases}

    first = sweep()
    try:
        model.set_precision("fp32")
        second = sweep()
    finally:
        model.set_precision("f16x2")
    third = sweep()
    for lid in xs:
        assert torch.isfinite(first[lid]).all()
        assert torch.equal(first[lid], third[lid]), f"layer {lid}: f16x2 output changed after a round trip through fp32"
        err = rel_rms(first[lid], second[lid])
        assert err < ACT_TOL, f"layer {lid}: f16x2 and fp32 differ by rel rms {err:.3e}"


def test_same_launch_twice_is_bit_identical(base_f16x2):
    """C = 144 encoder (paired, two heads per tile) and C = 72 decoder (one head over two tiles, halves paired)."""
    model, orc, g, cfg = base_f16x2
    lib, hd = _h(model)
    cases = {c[1]: c for c in _layer_cases(cfg)}
    torch.manual_seed(59)
    B, W = 3, 22
    for pfx, want in (("encoder.blocks.3.", (144, 24)), ("decoder.blocks.4.", (72, 3))):
        lid, _, C, nH, scale, H = cases[pfx]
        assert (C, nH) == want
        x = torch.randn(B, H * W, C)
        shape = _out_shape(B, H, W, C, scale, cfg, lid)
        y0, _ = _run_layer(lib, hd, lid, x, B, H, W, shape)
        y1, _ = _run_layer(lib, hd, lid, x, B, H, W, shape)
        assert torch.isfinite(y0).all() and torch.equal(y0, y1), f"{pfx}: two launches differ"
