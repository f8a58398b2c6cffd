"""TEST INFRASTRUCTURE -- the encoder's and the quantiser's parameter gradients of the DAC baseline (esc.baselines.DAC.encode after
set_encode_trainable): generates tests/golden/dac_encode_param_grad.npz by running the REAL reference DAC.encode
(baselines/descript/dac/model/dac.py:209-247 of the reference repository, with nn/quantize.py:58-70, 173-198 and nn/layers.py:5-33) in eval mode
under torch autograd on the CPU in float64, with the name-keyed weights of esc.synth.dac_tensor and every encoder and quantiser parameter
requiring a gradient.  Run in the build container only:

    python tools/gen_dac_encode_param_grad_golden.py [REFERENCE_ROOT]

Per configuration (tests/dac_encode_grad_util.FIXTURE_CASES), with the seeded audio x and the seeded cotangents on z, latents and the commitment
loss of tests/golden/dac_encode_grad.npz (not stored again), the file holds the seeded cotangent on the codebook loss, the codes the reference
chose and the float64 gradient of
sum(z * w_z) + sum(latents * w_lat) + cm * w_cm + cb * w_cb with respect to the encoder's and the quantiser's parameters: every tensor in full
for dac_syn; for dac_tiny every bias, weight_g and alpha in full and for each weight_v and codebook.weight its norm and its values at a seeded
index set (tests/dac_encode_param_grad_util.sample_index).  The float64 restatement of tests/dac_encode_param_grad_util.py must agree with the
reference on every tensor (asserted); tests/test_dac_encode_param_grad_host.py re-checks it from the file.  Data only; no reference source is
stored.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "efficient-speech-codec_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import dac_encode_grad_util as eu  # noqa: E402
import dac_encode_param_grad_util as qu  # noqa: E402
from gen_dac_golden import load_reference_dac  # noqa: E402


def reference_grads(mod, name, x, cot, n):
    model = mod.DAC(**eu.config(name)).eval()
    model.load_state_dict(eu.state_dict(name), strict=True)
    model = model.to(torch.float64)
    params = {}
    for k, p in model.named_parameters():
        p.requires_grad_(k.startswith(("encoder.", "quantizer.")))
        if p.requires_grad:
            params[k] = p
    seen = {}

    def fn(xt):
        z, codes, latents, cm, cb = model.encode(xt, n)
        seen["codes"] = codes.detach().numpy()
        return {"z": z, "latents": latents, "cm": cm, "cb": cb}

    return qu.grads_of(fn, params, x, cot, torch.float64), seen["codes"]


def main():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_shims
    ref_root = sys.argv[1] if len(sys.argv) > 1 else ref_shims.REFERENCE_ROOT
    torch.set_num_threads(8)
    mod = load_reference_dac(ref_root)
    out = {}
    for name, (B, L, n) in qu.FIXTURE_CASES.items():
        x, cot = qu.inputs(name, B, L, n)
        ref, codes = reference_grads(mod, name, x, cot, n)
        own = qu.oracle(name, x, cot, n)
        assert list(ref) == list(own) == qu.encode_keys(eu.state_dict(name)), "the reference's parameters are not the state_dict's, in order"
        assert np.array_equal(eu.oracle_codes(name, x, n), codes), f"{name}: the restatement chooses other codes than the reference"
        worst = 0.0
        for k, g in ref.items():
            assert g is not None and own[k] is not None and g.shape == own[k].shape and np.any(g != 0), k
            e = eu.rel_l2(own[k], g)
            worst = max(worst, e)
            assert e < 1e-12, f"{name} {k}: the float64 restatement differs from the reference by {e:.3e}"
        out[f"{name}_w_cb"], out[f"{name}_codes"] = np.array(cot["cb"]), codes.astype(np.int16)
        stored, norms = 0, []
        for k, g in ref.items():
            if qu.kind(k) in qu.SAMPLED.get(name, ()):
                idx = qu.sample_index(k, g.size)
                norms.append(np.linalg.norm(g.ravel()))
                out[f"{name}_s/{k}"] = g.ravel()[idx]
                stored += len(idx) + 1
            else:
                out[f"{name}_g/{k}"] = g
                stored += g.size
        assert len(norms) == len(qu.sampled_keys(name, list(ref)))
        if norms:
            out[f"{name}_norms"] = np.array(norms)
        print(f"[{name}] x {x.shape} n {n}  {len(ref)} tensors, {sum(g.size for g in ref.values())} values, {stored} stored;  "
              f"restatement f64 vs reference: worst tensor {worst:.3e}")
    path = os.path.join(eu.GOLD, "dac_encode_param_grad.npz")
    np.savez_compressed(path, **out)
    sz = os.path.getsize(path)
    print(f"   wrote {path} ({sz / 1e3:.0f} kB)")
    assert sz < 508_000, "fixture above the largest DAC fixture (508 kB)"


if __name__ == "__main__":
    main()
