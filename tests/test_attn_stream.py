"""The two-term (f16x2) weight streams of the fused attention and of PatchMerge / PatchSplit: dense layout (max(2 KS, KK) fragments per attention tile,
2 KS per row-GEMM output tile) in an allocation that keeps the three-term size, so that escx_set_precision can re-pack either form in place.

Every case drives escx_transformer_layer on the layer list of test_gpu_parity.py: head mappings 0, 1 and 2, the packed H = 2 kernel, shifted and unshifted
blocks, PatchMerge and PatchSplit are all on the path.  Tolerances are the project's own: ACT_TOL against the float32 oracle, and
device error <= 1.1 x the oracle's float32 error + 1e-7 against its float64 evaluation (test_layer_accuracy_against_fp64)."""
import ctypes

import pytest
import torch

from gpu_util import build_models, rel_rms
from esc import _native
from test_gpu_parity import ACT_TOL, _h, _layer_cases, _ptr

pytestmark = pytest.mark.gpu


def _run_layer(lib, hd, lid, x, B, H, W, out_shape):
    y = torch.empty(out_shape, device="cuda")
    Hn = ctypes.c_int()
    xg = x.cuda()
    _native.check(lib.escx_transformer_layer(hd, lid, _ptr(xg), B, H, W, _ptr(y), ctypes.byref(Hn), None))
    return y.cpu(), Hn.value


def _out_shape(B, H, W, C, scale, cfg, lid):
    """(B, H' * W, C') of a layer: "down" halves H (odd H rounds up) and moves to the next width, "up" doubles H and moves to the previous one."""
    h = cfg["h_dims"]
    n = len(h)
    if scale == "down":
        return (B, ((H + 1) // 2) * W, h[lid])            # encoder.blocks.i is layer 1 + i and ends at h[i + 1]
    if scale == "up":
        return (B, 2 * H * W, h[::-1][lid - n + 1])       # decoder.blocks.j is layer n + j and ends at reversed h[j + 1]
    return (B, H * W, C)


@pytest.fixture(scope="module")
def base_f16x2():
    return build_models("base", "f16x2")


@pytest.mark.parametrize("W", [20, 22])
def test_accuracy_with_partial_workgroups(base_f16x2, W):
    """f16x2, B = 3: an odd window count at every scale (the last workgroup, wave and packed pair are partial), W % 4 = 2 adds padded window slots.
    Every layer of ESC-Base against the oracle in float64, bound of test_layer_accuracy_against_fp64 (which runs W = 20, B = 2 only)."""
    from oracle import esc_oracle as O
    model, orc, g, cfg = base_f16x2
    lib, hd = _h(model)
    assert model.precision == "f16x2"
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in orc.sd.items()}
    torch.manual_seed(29)
    B = 3
    for lid, pfx, C, nH, scale, H in _layer_cases(cfg):
        x = torch.randn(B, H * W, C)
        ref64, Hr, _ = O.transformer_layer(x.double(), H, W, sd64, pfx, nH, cfg["swin_depth"], cfg["window_size"], scale)
        ref32, _, _ = O.transformer_layer(x, H, W, orc.sd, pfx, nH, cfg["swin_depth"], cfg["window_size"], scale)
        y, Hn = _run_layer(lib, hd, lid, x, B, H, W, ref32.shape)
        assert Hn == Hr
        e_dev, e_cpu = rel_rms(y.double(), ref64), rel_rms(ref32.double(), ref64)
        print(f"[stream fp64 W={W}] layer {lid:2d} {pfx:22s} C={C:3d}: device {e_dev:.2e}   reference float32 {e_cpu:.2e}   ratio {e_dev / max(e_cpu, 1e-30):.2f}")
        assert e_dev <= 1.1 * e_cpu + 1e-7, f"layer {lid} ({pfx}) W={W}: device error {e_dev:.3e} vs float32 reference error {e_cpu:.3e}"


def test_group_split_on_and_off(monkeypatch):
    """The head-group split (three workgroups per window block, each on a third of the head groups of the stream) against the unsplit walk, on the layers whose
    maps are small enough for it (C = 192, C = 384): both walks read the same image, so they must agree to summation order.  ESCX_ATTN_GS_TOKENS is read when
    the handle is created."""
    outs = {}
    for arm, val in (("default", None), ("off", "0")):
        if val is None:
            monkeypatch.delenv("ESCX_ATTN_GS_TOKENS", raising=False)
        else:
            monkeypatch.setenv("ESCX_ATTN_GS_TOKENS", val)
        model, orc, g, cfg = build_models("base", "f16x2")
        lib, hd = _h(model)
        torch.manual_seed(31)
        for W in (20, 22):
            for lid, pfx, C, nH, scale, H in _layer_cases(cfg):
                if C not in (192, 384):
                    continue
                x = torch.randn(3, H * W, C)
                outs.setdefault((lid, W), {})[arm], _ = _run_layer(lib, hd, lid, x, 3, H, W, _out_shape(3, H, W, C, scale, cfg, lid))
        del model
    assert len(outs) == 6                       # encoder.blocks.4, decoder.blocks.0, decoder.blocks.1 at two widths
    for (lid, W), o in outs.items():
        assert torch.isfinite(o["default"]).all()
        err = rel_rms(o["off"], o["default"])
        assert err < ACT_TOL, f"layer {lid} W={W}: split on / off differ by rel rms {err:.3e}"


def test_both_layouts_share_one_buffer():
    """set_precision re-packs the images in place: f16x2 (dense two-term layout) -> bf16x3 (three-term layout, the whole allocation) -> f16x2 on one handle.
    First and third outputs bit-identical, the bf16x3 output bit-identical to a fresh bf16x3 handle's.  C = 96 and 144 (merge layers), C = 384 (packed kernel,
    a split layer), C = 144 split."""
    model, orc, g, cfg = build_models("base", "f16x2")
    fresh, _, _, _ = build_models("base", "bf16x3")
    lib, hd = _h(model)
    _, hd3 = _h(fresh)
    cases = [c for c in _layer_cases(cfg) if c[0] in (3, 4, 6, 8)]
    assert [(c[2], c[4]) for c in cases] == [(96, "down"), (144, "down"), (384, "up"), (144, "up")]
    torch.manual_seed(37)
    W, B = 22, 3
    xs = {lid: torch.randn(B, H * W, C) for lid, pfx, C, nH, scale, H in cases}

    def sweep(handle):
        return {lid: _run_layer(lib, handle, lid, xs[lid], B, H, W, _out_shape(B, H, W, C, scale, cfg, lid))[0] for lid, pfx, C, nH, scale, H in cases}

    first = sweep(hd)
    model.set_precision("bf16x3")
    second = sweep(hd)
    model.set_precision("f16x2")
    third = sweep(hd)
    ref3 = sweep(hd3)
    for lid in xs:
        assert torch.isfinite(first[lid]).all()
        assert torch.equal(first[lid], third[lid]), f"layer {lid}: f16x2 output changed after a round trip through bf16x3"
        assert torch.equal(second[lid], ref3[lid]), f"layer {lid}: bf16x3 after f16x2 differs from a fresh bf16x3 handle"
        assert not torch.equal(first[lid], second[lid])         # the modes really are different arithmetic


@pytest.mark.parametrize("which,W", [("tiny", 32), ("tiny", 30), ("base", 22)])
def test_narrow_layers_in_two_term_mode(which, W, request):
    """The narrow widths in f16x2: the C = 45 layers of ESC-Base (3 head groups, two windows per wave, tile of max(2 KS, KK) = 4 fragments) and
    every layer of the tiny configuration (no split-operand instantiation: the fp32 kernels), comparison of test_every_transformer_layer."""
    from oracle import esc_oracle as O
    model, orc, g, cfg = request.getfixturevalue("base_f16x2") if which == "base" else build_models("tiny", "f16x2")
    lib, hd = _h(model)
    torch.manual_seed(41)
    n = 0
    for lid, pfx, C, nH, scale, H in _layer_cases(cfg):
        if which == "base" and C != 45:
            continue
        x = torch.randn(2, H * W, C)
        ref, Hr, _ = O.transformer_layer(x, H, W, orc.sd, pfx, nH, cfg["swin_depth"], cfg["window_size"], scale)
        y, Hn = _run_layer(lib, hd, lid, x, 2, H, W, ref.shape)
        assert Hn == Hr
        err = rel_rms(y, ref)
        assert err < ACT_TOL, f"{which} layer {lid} ({pfx}) H={H} W={W}: rel rms {err:.3e}"
        n += 1
    assert n == (3 if which == "base" else len(_layer_cases(cfg)))
