"""TEST INFRASTRUCTURE -- fixture of the discriminator WITH the multi-scale branch (MSD, `rates`) from the REAL reference Discriminator and
GANLoss (imported through oracle/ref_shims.py, as oracle/gen_disc_alt_golden.py does), on name-keyed synthetic weights.

    python tools/gen_msd_golden.py         # writes tests/golden/msd.npz + msd_manifest.json   (CPU, where the reference is installed)

Two things the reference leaves to libraries that are not installed are supplied here:
  * `AudioSignal.resample` (audiotools -> julius.resample_frac): the stand-in gets the resampler of tests/msd_util.py.  The
    fixture therefore pins the MSD's convolutions, their order, the parameter names and the losses against the reference, NOT the resampler:
    that boundary is unpinned, like the matched-stride STFT of oracle/gen_disc_golden.py.
  * The reference's GANLoss averages every map over dim=[1, 2, 3], which a (B, C, T) map does not have: the MSD maps are handed to it with a
    trailing unit dimension (the same mean over everything but the batch).  The stored shapes are the reference's own 3-D ones.
"""
import json, os, sys
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gen_golden as gg  # noqa: E402
import gen_disc_golden as gd  # noqa: E402
import msd_util as mu  # noqa: E402

CFG, B, L = mu.CFG_A, mu.B_A, mu.L_A


def main():
    torch.manual_seed(0); torch.set_num_threads(8)
    gg.ref_shims.install()
    gd.install_audiotools()
    AudioSignal = sys.modules["audiotools"].AudioSignal

    def resample(self, sample_rate):
        assert self.sample_rate % sample_rate == 0
        self.audio_data = mu.resample(self.audio_data, self.sample_rate // sample_rate)
        self.sample_rate = sample_rate
        return self
    AudioSignal.resample = resample
    import importlib
    D = importlib.import_module("esc.models.discriminator")
    G = importlib.import_module("esc.modules.loss.gan_loss")
    D.AudioSignal, D.STFTParams = AudioSignal, sys.modules["audiotools"].STFTParams
    disc = D.Discriminator(**{**CFG, "bands": [tuple(b) for b in CFG["bands"]]})
    manifest = {k: list(v.shape) for k, v in disc.state_dict().items()}
    disc.load_state_dict({k: torch.from_numpy(v) for k, v in gd.synth_disc_state(manifest).items()})

    class FourD(torch.nn.Module):               # see the module docstring
        def __init__(self, d):
            super().__init__(); self.d = d

        def forward(self, x):
            return [[t.unsqueeze(-1) if t.dim() == 3 else t for t in f] for f in self.d(x)]
    gan = G.GANLoss(FourD(disc))
    real = torch.from_numpy(gg.synth.pcm_to_float(np.stack([gg.synth.voiced_clip_int16(f"msd-real-{i}", L) for i in range(B)])))
    fake = (0.7 * real + torch.from_numpy(gg.synth.pcm_to_float(np.stack([gg.synth.noise_clip_int16(f"msd-fake-{i}", L, amp=0.03) for i in range(B)])))).requires_grad_(True)
    keys = [k for k, _ in disc.named_parameters()]
    out = {"cfg_json": np.array(json.dumps(CFG)), "keys_json": np.array(json.dumps(keys)), "n_samples": np.int64(L), "batch": np.int64(B)}
    disc.zero_grad()
    ld = gan.discriminator_loss(fake, real)
    ld.mean().backward()
    params = dict(disc.named_parameters())
    out["disc_loss"] = ld.detach().numpy()
    out["disc_gnorm"] = np.array([float(params[k].grad.double().norm()) for k in keys])
    disc.zero_grad(); fake.grad = None
    lg, lf = gan.generator_loss(fake, real)
    (lg + 2.0 * lf).mean().backward()
    out["gen_loss"], out["feat_loss"], out["d_fake"] = lg.detach().numpy(), lf.detach().numpy(), fake.grad.numpy().astype(np.float32)
    with torch.no_grad():
        fm = disc(fake.detach().unsqueeze(1))
    shapes = [[list(t.shape) for t in f] for f in fm]
    out["fmap_shapes_json"] = np.array(json.dumps(shapes))
    out["fmap_rms"] = np.array([[float(t.double().pow(2).mean().sqrt()) for t in f] + [0.0] * (32 - len(f)) for f in fm])
    print("disc", out["disc_loss"], "gen", out["gen_loss"], "feat", out["feat_loss"], [len(f) for f in fm])
    np.savez_compressed(os.path.join(gg.GOLD, "msd.npz"), **out)
    json.dump({"config": CFG, "batch": B, "n_samples": L, "state_dict": manifest, "keys": keys, "fmap_shapes": shapes,
               "disc_loss": out["disc_loss"].tolist(), "gen_loss": out["gen_loss"].tolist(), "feat_loss": out["feat_loss"].tolist()},
              open(os.path.join(gg.GOLD, "msd_manifest.json"), "w"), indent=0)


if __name__ == "__main__":
    main()
