"""Data plumbing of the evaluation harness (reference: scripts/utils.py:27-46,75-91), wav I/O through scipy."""
import glob
import warnings

import numpy as np
import torch
import yaml
from scipy.io import wavfile
from torch.utils.data import Dataset


def load_wav(path):
    sr, pcm = wavfile.read(path)
    if pcm.dtype == np.int16:
        x = pcm.astype(np.float32) / 32768.0
    elif pcm.dtype == np.int32:
        x = pcm.astype(np.float32) / 2147483648.0
    else:
        x = pcm.astype(np.float32)
    x = torch.from_numpy(np.atleast_2d(x.T if x.ndim == 2 else x))          # (channels, L) like torchaudio.load
    return x, sr


class EvalSet(Dataset):
    """utils.py:27-40 -- first channel, last 80 samples dropped (so that a 3 s file gives an even frame count)."""

    def __init__(self, eval_folder_path):
        self.testset_files = sorted(glob.glob(f"{eval_folder_path}/*.wav")) or sorted(glob.glob(f"{eval_folder_path}/*/*.wav"))
        self.testset_files = self.testset_files[:180000]

    def __len__(self):
        return len(self.testset_files)

    def __getitem__(self, i):
        x, _ = load_wav(self.testset_files[i])
        return x[0, :-80]


RAGGED_MIN_SAMPLES = 1024          # the mel distance's 2048-sample window reflects 1024 samples: an evaluated clip is longer


def snap_length(model, L):
    """The longest length <= L that `model` reconstructs at full length (idempotent).  ESC gives hop * (patch_t * W - 1) samples for W latent frames and
    takes W in multiples of `overlap`: 48000 -> 47920 (EvalSet's [:-80]), 20000 -> 19760, 30000 -> 30000.  The DAC adapter (DacEvalModel) fits
    every length: L itself."""
    if getattr(model, "dac", None) is not None:
        return int(L)
    hop, pt, ov = model.hop_length, model.cfg["patch_size"][1], model.cfg["overlap"]
    W = ((1 + int(L) // hop) // pt) // ov * ov
    return max(hop * (pt * W - 1), 0)


class RaggedEvalSet(Dataset):
    """Whole utterances of different lengths: item i is (first channel trimmed to its snapped length, file index), longest file first, so that a
    DataLoader without shuffling forms batches of similar lengths.  The file index counts the kept files in name order (EvalSet's order), which is
    the order results are reported in.  A file whose snapped length is not above 1024 samples is skipped with a warning that names it."""

    def __init__(self, eval_folder_path, model):
        files = sorted(glob.glob(f"{eval_folder_path}/*.wav")) or sorted(glob.glob(f"{eval_folder_path}/*/*.wav"))
        self.testset_files, self.lengths = [], []
        for f in files[:180000]:
            n = snap_length(model, wavfile.read(f, mmap=True)[1].shape[0])
            if n <= RAGGED_MIN_SAMPLES:
                warnings.warn(f"{f}: {n} samples after snapping to the model's lengths, not more than {RAGGED_MIN_SAMPLES}: skipped")
                continue
            self.testset_files.append(f)
            self.lengths.append(n)
        self.order = sorted(range(len(self.lengths)), key=lambda i: -self.lengths[i])        # stable: equal lengths keep the name order

    def __len__(self):
        return len(self.order)

    def __getitem__(self, i):
        k = self.order[i]
        x, _ = load_wav(self.testset_files[k])
        return x[0, :self.lengths[k]], k


def ragged_collate(items):
    """[(waveform (L_b,), file index)] -> (x (B, max L_b) zero-padded, lengths [L_b], indices)."""
    lengths = [int(x.shape[-1]) for x, _ in items]
    out = torch.zeros(len(items), max(lengths, default=0), dtype=torch.float32)
    for b, (x, _) in enumerate(items):
        out[b, :lengths[b]] = x
    return out, lengths, [int(k) for _, k in items]


def in_file_order(values_by_index):
    """Per-file values stored by file index (batches come longest first) -> the list in file order."""
    return [values_by_index[k] for k in sorted(values_by_index)]


def read_yaml(pth):
    with open(pth, "r") as f:
        return yaml.safe_load(f)
