"""TEST INFRASTRUCTURE -- the audio gradient of the DAC baseline's encoder and quantiser (esc.baselines.DAC.encode under autograd): generates
tests/golden/dac_encode_grad.npz by running the REAL reference DAC.encode (baselines/descript/dac/model/dac.py:209-247 of the reference
repository, with nn/quantize.py:58-70, 173-198) in eval mode under torch autograd on the CPU, in float64 and in float32, with the name-keyed
weights of esc.synth.dac_tensor.  Run in the build container only:

    python tools/gen_dac_encode_grad_golden.py [REFERENCE_ROOT]

Per configuration (dac_syn, dac_tiny; tests/dac_encode_grad_util.FIXTURE_CASES) the file holds the seeded audio x (B, 1, L), the seeded
cotangents on z, latents and the commitment loss, d_x = the three pulled back to the audio in float64, the codes the reference chose, and the
reference's own float32-against-float64 relative error of d_x.  Inputs are float32-representable values stored as float64.  The restatement
of tests/dac_encode_grad_util.py in float64 must agree with the reference here (asserted); tests/test_dac_encode_grad_host.py re-checks it
from the file.  Data only; no reference source is stored.
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
from gen_dac_golden import load_reference_dac  # noqa: E402


def reference_grad(mod, name, x, cot, n, dtype):
    model = mod.DAC(**eu.config(name)).eval()
    model.load_state_dict(eu.state_dict(name), strict=True)
    model = model.to(dtype)
    for p in model.parameters():
        p.requires_grad_(False)
    seen = {}

    def fn(xt):
        z, codes, latents, cm, _ = model.encode(xt, n)
        seen["codes"] = codes.detach().numpy()
        return {"z": z, "latents": latents, "cm": cm}

    return eu.grad_of(fn, x, cot, dtype), seen["codes"]


def main():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_shims
    ref_root = sys.argv[1] if len(sys.argv) > 1 else ref_shims.REFERENCE_ROOT
    torch.set_num_threads(8)
    mod = load_reference_dac(ref_root)
    out = {}
    for name, (B, L, n) in eu.FIXTURE_CASES.items():
        x, cot = eu.inputs(name, B, L, n)
        d64, codes = reference_grad(mod, name, x, cot, n, torch.float64)
        d32, codes32 = reference_grad(mod, name, x, cot, n, torch.float32)
        own = eu.rel_l2(eu.oracle(name, x, cot, n), d64)
        assert own < 1e-12, f"{name}: the float64 restatement differs from the reference by {own:.3e}"
        assert np.array_equal(eu.oracle_codes(name, x, n), codes), f"{name}: the restatement chooses other codes than the reference"
        out[f"{name}_x"], out[f"{name}_w_z"], out[f"{name}_w_latents"], out[f"{name}_w_cm"] = x, cot["z"], cot["latents"], np.array(cot["cm"])
        out[f"{name}_d_x"], out[f"{name}_codes"] = d64, codes.astype(np.int16)
        out[f"{name}_ref_f32_err"] = np.array(eu.rel_l2(d32, d64))
        parts = {k: np.linalg.norm(eu.oracle(name, x, {k: w}, n)) for k, w in cot.items()}
        print(f"[{name}] x {x.shape} n {n}  |d_x| {np.linalg.norm(d64):.4g} (z {parts['z']:.3g}, latents {parts['latents']:.3g}, commitment {parts['cm']:.3g})  "
              f"reference f32 vs f64 {eu.rel_l2(d32, d64):.3e} (codes equal: {np.array_equal(codes, codes32)})  restatement f64 vs reference {own:.3e}")
    path = os.path.join(eu.GOLD, "dac_encode_grad.npz")
    np.savez_compressed(path, **out)
    sz = os.path.getsize(path)
    print(f"   wrote {path} ({sz / 1e3:.0f} kB)")
    assert sz < 200_000, "fixture above the 200 kB it is meant to stay under"


if __name__ == "__main__":
    main()
