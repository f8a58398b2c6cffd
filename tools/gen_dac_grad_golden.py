"""TEST INFRASTRUCTURE -- the latent gradient of the DAC baseline's decoder (esc.baselines.DAC.decode under autograd): generates
tests/golden/dac_grad.npz by running the REAL reference DAC.decode (baselines/descript/dac/model/dac.py:249-266 of the reference repository)
under torch autograd on the CPU, in float64 and in float32, with the name-keyed weights of esc.synth.dac_tensor.  Run in the build container only:

    python tools/gen_dac_grad_golden.py [REFERENCE_ROOT]

Per configuration (dac_syn, dac_tiny; tests/dac_grad_util.FIXTURE_CASES) the file holds a seeded latent z (B, D, T), a seeded cotangent
w (B, 1, samples), d_z = (d audio / d z)^T w in float64, and the reference's own float32-against-float64 relative error of d_z.  z and w are
float32-representable values stored as float64.  The restatement of tests/dac_util.py in float64 must agree with the reference here (asserted);
tests/test_dac_grad_host.py re-checks it from the file.  Data only; no reference source is stored.
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
import dac_grad_util as gu  # noqa: E402
from gen_dac_golden import load_reference_dac  # noqa: E402


def reference_grad(mod, name, z, w, dtype):
    model = mod.DAC(**gu.config(name)).eval()
    model.load_state_dict(gu.state_dict(name), strict=True)
    model = model.to(dtype)
    for p in model.parameters():
        p.requires_grad_(False)
    return gu.grad_of(model.decode, z, w, dtype)


def main():
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import ref_shims
    ref_root = sys.argv[1] if len(sys.argv) > 1 else ref_shims.REFERENCE_ROOT
    torch.set_num_threads(8)
    mod = load_reference_dac(ref_root)
    out = {}
    for name, (B, T) in gu.FIXTURE_CASES.items():
        z, w = gu.inputs(name, B, T)
        d64 = reference_grad(mod, name, z, w, torch.float64)
        d32 = reference_grad(mod, name, z, w, torch.float32)
        own = gu.rel_l2(gu.oracle(name, z, w), d64)
        assert own < 1e-12, f"{name}: the float64 restatement differs from the reference by {own:.3e}"
        out[f"{name}_z"], out[f"{name}_w"], out[f"{name}_d_z"] = z, w, d64
        out[f"{name}_ref_f32_err"] = np.array(gu.rel_l2(d32, d64))
        print(f"[{name}] z {z.shape}  w {w.shape}  |d_z| {np.linalg.norm(d64):.4g}  zeros {int((d64 == 0).sum())}  reference f32 vs f64 {gu.rel_l2(d32, d64):.3e}  "
              f"restatement f64 vs reference {own:.3e}")
    path = os.path.join(gu.GOLD, "dac_grad.npz")
    np.savez_compressed(path, **out)
    sz = os.path.getsize(path)
    print(f"   wrote {path} ({sz / 1e3:.0f} kB)")
    assert sz < 200_000, "fixture above the 200 kB it is meant to stay under"


if __name__ == "__main__":
    main()
