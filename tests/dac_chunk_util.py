"""Torch restatement of the DAC baseline with every convolution unpadded (the reference after `model.padding = False`, base.py:64-80) and of
the chunk schedule's window batch, for tests/test_dac_chunked*.py and tools/gen_dac_chunk_golden.py.  It extends tests/dac_util.py's DacRef:
F.conv1d without padding, the ResidualUnit's skip cropped by 3 * dilation on each side (dac.py:35-40), conv_transpose1d(padding=0).  The
generator pins it to the real reference on the CPU; on the GPU it is a second oracle for the native path."""
import json

import numpy as np
import torch
import torch.nn.functional as F

import dac_util as du

# (fixture key, configuration fixture, win_duration, signal length)
CASES = (("syn769", "dac_syn", 0.048, 769), ("syn1016", "dac_syn", 0.048, 1016), ("syn1017", "dac_syn", 0.048, 1017), ("tiny16001", "dac_tiny", 1.0, 16001))
GEOMETRY_NS = {"dac_syn": (520, 640, 768, 1024), "dac_tiny": (16000,), "dac_base": (16000,)}


def clip_tag(key):
    return f"dac-chunk-{key}"


class DacRefNoPad(du.DacRef):
    """DacRef with padding 0 everywhere; the quantiser (1x1 projections) is inherited unchanged."""

    def _res(self, x, p, dil):
        y = self._conv(self._snake(x, p + "block.0."), p + "block.1.", dilation=dil)
        y = self._conv(self._snake(y, p + "block.2."), p + "block.3.")
        pad = (x.shape[-1] - y.shape[-1]) // 2
        assert pad == 3 * dil and y.shape[-1] == x.shape[-1] - 6 * dil
        return x[..., pad:-pad] + y

    def encoder(self, x):
        r = self.cfg["encoder_rates"]
        x = self._conv(x, "encoder.block.0.")
        for i, s in enumerate(r):
            p = f"encoder.block.{i + 1}.block."
            for j, d in enumerate((1, 3, 9)):
                x = self._res(x, f"{p}{j}.", d)
            x = self._conv(self._snake(x, f"{p}3."), f"{p}4.", stride=s)
        n = len(r)
        return self._conv(self._snake(x, f"encoder.block.{n + 1}."), f"encoder.block.{n + 2}.")

    def decoder(self, z):
        r = self.cfg["decoder_rates"]
        x = self._conv(z, "decoder.model.0.")
        for i, s in enumerate(r):
            p = f"decoder.model.{i + 1}.block."
            x = self._snake(x, f"{p}0.")
            x = F.conv_transpose1d(x, self._w(f"{p}1."), self.sd[f"{p}1.bias"], stride=s)
            for j, d in enumerate((1, 3, 9)):
                x = self._res(x, f"{p}{j + 2}.", d)
        n = len(r)
        return torch.tanh(self._conv(self._snake(x, f"decoder.model.{n + 1}."), f"decoder.model.{n + 2}."))


def chunk_batch(x, delay, hop, n_samples):
    """The windows base.py:197, 206-208 cuts: x (rows, 1, nt) zero-padded by `delay` on both sides, one window of n_samples from every
    multiple of hop below nt, a short last one zero-padded on the right -> (rows * n_chunks, 1, n_samples), row-major (row, chunk)."""
    rows, _, nt = x.shape
    xp = F.pad(x, (delay, delay))
    wins = []
    for i in range(0, nt, hop):
        w = xp[..., i:i + n_samples]
        wins.append(F.pad(w, (0, n_samples - w.shape[-1])))
    return torch.stack(wins, 1).reshape(rows * len(wins), 1, n_samples)


def unchunk_codes(codes, rows):
    """(rows * n_chunks, n, T) -> (rows, n, n_chunks * T): the reference's torch.cat(codes, dim=-1)."""
    B, n, T = codes.shape
    return codes.reshape(rows, B // rows, n, T).permute(0, 2, 1, 3).reshape(rows, n, -1)


def config_of(golden, name):
    return json.loads(str(golden(name)["config_json"]))


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


def rel_rms(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.sqrt(((a - b) ** 2).mean()) / max(np.sqrt((b ** 2).mean()), 1e-30))
