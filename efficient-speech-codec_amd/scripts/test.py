"""Evaluation CLI, counterpart of the reference's scripts/test.py:23-82: every bitrate (num_streams 1..max), metrics per
clip, codebook utilisation, `perf_stats.json` with the same layout.

    python -m scripts.test --eval_folder_path ./eval --batch_size 36 --model_path ./esc9kbps --device cuda
    python -m scripts.test --eval_folder_path ./eval --synthetic base --device cuda          # no checkpoint available
    python -m scripts.test --eval_folder_path ./eval --dac_path ./dac/weights.pth --n_quantizers 3,6,9,12,15,18 --one_pass      # the DAC baseline

`--one_pass` encodes every batch once and decodes it at each bitrate (both codecs emit prefix codes): the same table, bit for bit, as the
default sweep that runs the whole forward once per bitrate.

    python -m scripts.test --eval_folder_path ./utterances --ragged --batch_size 8 --model_path ./esc9kbps      # whole utterances of different lengths

`--ragged` evaluates a folder whose files differ in length in batches: every file is trimmed to the longest length the model reconstructs in full
(snap_length), batches are formed longest first and run through the codecs' `lengths` calls and the length-aware HIP metrics of esc.metrics, and every
file gets the numbers of the reference's batch-size-1 loop.  `--native_metrics` alone swaps the metric classes on the uniform path.
"""
import inspect
import math
import argparse
import json
import os
import sys

import numpy as np
import torch
from torch.utils.data import DataLoader, default_collate

from esc.models import make_model
from .metrics import EntropyCounter, MelSpectrogramDistance, SISDR
from .utils import EvalSet, RaggedEvalSet, in_file_order, ragged_collate, read_yaml


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--eval_folder_path", type=str, required=True)
    p.add_argument("--batch_size", type=int, default=1)
    p.add_argument("--model_path", type=str, default=None, help="folder with config.yaml and model.pth")
    p.add_argument("--synthetic", type=str, default=None, help="base|large|tiny|rvq_tiny, or dac_syn|dac_tiny|dac_base for the DAC baseline: config "
                                                                "from tests/golden with name-keyed synthetic weights")
    p.add_argument("--dac_path", type=str, default=None, help="DAC baseline checkpoint (weights.pth, esc.baselines.DAC.load)")
    p.add_argument("--n_quantizers", type=str, default=None, help="DAC: codebook counts of the evaluated bitrates, e.g. 3,6,9,12,15,18")
    p.add_argument("--one_pass", action="store_true", help="encode each batch once for the whole sweep (eval_epoch_one_pass)")
    p.add_argument("--ragged", action="store_true", help="files of different lengths in one batch: RaggedEvalSet, esc.metrics, eval_epoch_ragged")
    p.add_argument("--native_metrics", action="store_true", help="MelDistance / SISDR / utilisation from esc.metrics (HIP) instead of scripts.metrics")
    p.add_argument("--save_path", type=str, default=None)
    p.add_argument("--device", type=str, default="cuda")
    return p.parse_args()


def _code_slots(model, s):
    """Code slots (axis 1 of "codes") a model emits at the s-th evaluated bitrate: s itself for ESC / RVQCodecs, n_s codebooks for DacEvalModel."""
    return model.code_slots(s) if isinstance(model, DacEvalModel) else s


class DacEvalModel(torch.nn.Module):
    """The DAC baseline (esc.baselines.DAC) behind the interface eval_epoch drives: bitrate s in 1..max_streams is n_quantizers[s - 1] codebooks,
    `model(x=x, x_feat=None, num_streams=s)` returns {"recon_audio": (B, L), "codes": (B, n_s, 1, T)} from DAC.forward (one code group, so
    EntropyCounter(num_groups=1) counts it as it is)."""

    def __init__(self, dac, n_quantizers=None):
        super().__init__()
        self.dac = dac
        self.n_quantizers = self.default_n_quantizers(dac.n_codebooks) if n_quantizers is None else [int(n) for n in n_quantizers]
        if not self.n_quantizers or any(b <= a for a, b in zip(self.n_quantizers, self.n_quantizers[1:])) or \
                not 1 <= self.n_quantizers[0] <= self.n_quantizers[-1] <= dac.n_codebooks:
            raise ValueError(f"n_quantizers {self.n_quantizers}: strictly increasing codebook counts in [1, {dac.n_codebooks}] expected")
        self.train(dac.training)                        # the adapter is in the mode of the model it wraps

    @staticmethod
    def default_n_quantizers(n_codebooks):
        """Six equal steps (3, 6, ..., 18 of 18 codebooks: the paper's 1.5 to 9 kbps) when 6 divides n_codebooks, else every codebook count."""
        step = n_codebooks // 6
        return [step * (i + 1) for i in range(6)] if n_codebooks % 6 == 0 else list(range(1, n_codebooks + 1))

    @property
    def max_streams(self):
        return len(self.n_quantizers)

    def code_slots(self, s):
        return self.n_quantizers[s - 1]

    @property
    def kbps_per_codebook(self):
        """frame_rate * log2(codebook_size) / 1000: 0.5 for the 16 kHz configurations (hop 320, 1024 entries)."""
        return self.dac.sample_rate / self.dac.hop_length * math.log2(self.dac.codebook_size) / 1000.0

    def kbps(self, s):
        return self.code_slots(s) * self.kbps_per_codebook

    @property
    def bps_per_stream(self):
        """eval_epoch prints s * bps_per_stream: exact when the counts are k, 2k, 3k, ...; None otherwise."""
        k = self.n_quantizers[0]
        return k * self.kbps_per_codebook if self.n_quantizers == [k * (i + 1) for i in range(len(self.n_quantizers))] else None

    @staticmethod
    def _fit(audio, length):
        """(B, 1, <= length) -> (B, length).  The decoder gives hop * T - 8 samples for rates [8, 5, 4, 2], so a clip whose length is a multiple
        of the hop comes back 8 samples short (dac.py:316 trims, it never pads): those are zero here, so that the metrics see equal lengths.
        EvalSet's clips (a whole number of hops minus 80 samples) are not affected."""
        return torch.nn.functional.pad(audio[:, 0], (0, length - audio.shape[-1]))

    def forward(self, x, x_feat, num_streams, lengths=None):
        out = self.dac(x[:, None], None, self.code_slots(num_streams)) if lengths is None else self.dac(x[:, None], None, self.code_slots(num_streams), lengths=lengths)
        return {"recon_audio": self._fit(out["audio"], x.shape[-1]), "codes": out["codes"][:, :, None]}

    def sweep(self, x, streams):
        """One encode for the bitrates `streams`: [(recon_audio (B, L), codes (B, n_s, 1, T)) per s], bitwise forward()'s."""
        L = x.shape[-1]
        ns = [self.code_slots(s) for s in streams]
        zs, codes, _ = self.dac.encode_sweep(self.dac.preprocess(x[:, None], None), ns)
        return [(self._fit(self.dac.decode(zs[r])[..., :L], L), codes[:, :n, None]) for r, n in enumerate(ns)]


def _sweep(model, x, streams):
    """[(recon_audio, codes) per s in `streams`] from one encode of x.  ESC / RVQCodecs: codes at max(streams), the first s streams decoded."""
    if isinstance(model, DacEvalModel):
        return model.sweep(x, streams)
    codes, feat_shape = model.encode(x, max(streams))
    return [(model.decode(codes[:, :s], feat_shape), codes[:, :s]) for s in streams]


def _bitrate_pass(model, batches, metric_funcs, e_counter, device, s):
    """One sweep of the evaluation set at `s` streams: per-clip metric values and the code utilisation of this bitrate."""
    scores = {name: [] for name in metric_funcs}
    e_counter.reset_stats(num_streams=_code_slots(model, s))
    for x in batches:
        x = x.to(device)
        out = model(x=x, x_feat=None, num_streams=s)
        for name, fn in metric_funcs.items():
            scores[name] += fn(x, out["recon_audio"]).tolist()
        e_counter.update(out["codes"])
    return scores, e_counter.compute_utilization()[0]


@torch.no_grad()
def eval_epoch(model, eval_loader, metric_funcs, e_counter, device, bps_per_stream, num_streams=None, verbose=True):
    """Counterpart of the reference's eval_epoch (scripts/test.py:23-55): the same arguments and the same result layout
    {metric: [mean at each evaluated bitrate, rounded to 4], "utilization": [...]}, bitrates = one (`num_streams`) or 1..max_streams.
    The model is put in eval mode for the sweep and its previous train/eval flag is restored afterwards (the reference forces
    train(); here a caller that evaluates an inference-only model keeps an inference-only model)."""
    was_training = model.training
    model.eval()
    streams = [num_streams] if num_streams is not None else list(range(1, model.max_streams + 1))
    table = {name: [] for name in metric_funcs}
    table["utilization"] = []
    try:
        for s in streams:
            scores, rate = _bitrate_pass(model, eval_loader, metric_funcs, e_counter, device, s)
            for name, vals in scores.items():
                table[name].append(round(float(np.mean(vals)), 4))
            table["utilization"].append(rate)
            if verbose:
                line = " | ".join(f"{name}: {np.mean(vals):.4f}" for name, vals in scores.items())
                print(f"Test Metrics at {s * bps_per_stream:.2f}kbps: {line} | utilization: {rate:.4f}")
    finally:
        model.train(was_training)
    return table


@torch.no_grad()
def eval_epoch_one_pass(model, eval_loader, metric_funcs, e_counter, device, bps_per_stream, num_streams=None, verbose=True):
    """eval_epoch with one encode per batch instead of one per (batch, bitrate): the same arguments and, bit for bit, the same table.  The eval
    forward equals decode(encode()), a lower bitrate's codes are a prefix of a higher one's, and DAC's running-sum snapshots equal its z at
    each count, so every (batch, bitrate) pair sees the tensors of the sequential sweep; metrics and utilisation are accumulated per bitrate in
    the sweep's order."""
    was_training = model.training
    model.eval()
    streams = [num_streams] if num_streams is not None else list(range(1, model.max_streams + 1))
    scores = [{name: [] for name in metric_funcs} for _ in streams]
    kept = []                                                   # each batch's codes at the highest bitrate (the others are prefixes)
    try:
        for x in eval_loader:
            x = x.to(device)
            outs = _sweep(model, x, streams)
            for i, (recon, _) in enumerate(outs):
                for name, fn in metric_funcs.items():
                    scores[i][name] += fn(x, recon).tolist()
            kept.append(outs[-1][1])
        table = {name: [] for name in metric_funcs}
        table["utilization"] = []
        for i, s in enumerate(streams):
            slots = _code_slots(model, s)
            e_counter.reset_stats(num_streams=slots)
            for codes in kept:
                e_counter.update(codes[:, :slots])
            rate = e_counter.compute_utilization()[0]
            for name, vals in scores[i].items():
                table[name].append(round(float(np.mean(vals)), 4))
            table["utilization"].append(rate)
            if verbose:
                line = " | ".join(f"{name}: {np.mean(vals):.4f}" for name, vals in scores[i].items())
                print(f"Test Metrics at {s * bps_per_stream:.2f}kbps: {line} | utilization: {rate:.4f}")
    finally:
        model.train(was_training)
    return table


def _takes_lengths(fn):
    return "lengths" in inspect.signature(fn.forward if isinstance(fn, torch.nn.Module) else fn).parameters


def _ragged_metric(fn, x, recon, lengths):
    """Per-clip values of one metric on a zero-padded batch: the length-aware metrics of esc.metrics take the batch; anything else (PESQ, on the
    host) is applied clip by clip to x[b, :L_b] and recon[b, :L_b]."""
    if _takes_lengths(fn):
        return fn(x, recon, lengths=lengths).tolist()
    return [float(fn(x[b:b + 1, :n], recon[b:b + 1, :n])[0]) for b, n in enumerate(lengths)]


@torch.no_grad()
def eval_epoch_ragged(model, eval_loader, metric_funcs, e_counter, device, bps_per_stream, num_streams=None, verbose=True):
    """eval_epoch over batches of clips of different lengths: `eval_loader` yields (x zero-padded, lengths, file indices) (ragged_collate), the model is
    called with `lengths`, the metrics get them too, and the counter skips the -1 filler of the codes.  Per-file values are stored by file index and
    averaged in file order, so the table does not depend on how the batches were formed; its layout is eval_epoch's.  A model without mixed-length
    batches raises its own NotImplementedError."""
    was_training = model.training
    model.eval()
    streams = [num_streams] if num_streams is not None else list(range(1, model.max_streams + 1))
    table = {name: [] for name in metric_funcs}
    table["utilization"] = []
    try:
        for s in streams:
            scores = {name: {} for name in metric_funcs}
            e_counter.reset_stats(num_streams=_code_slots(model, s))
            for x, lengths, indices in eval_loader:
                x = x.to(device)
                out = model(x=x, x_feat=None, num_streams=s, lengths=lengths)
                for name, fn in metric_funcs.items():
                    scores[name].update(zip(indices, _ragged_metric(fn, x, out["recon_audio"], lengths)))
                e_counter.update(out["codes"])
            rate = e_counter.compute_utilization()[0]
            means = {name: float(np.mean(in_file_order(vals))) for name, vals in scores.items()}
            for name, v in means.items():
                table[name].append(round(v, 4))
            table["utilization"].append(rate)
            if verbose:
                line = " | ".join(f"{name}: {v:.4f}" for name, v in means.items())
                print(f"Test Metrics at {s * bps_per_stream:.2f}kbps: {line} | utilization: {rate:.4f}")
    finally:
        model.train(was_training)
    return table


def _golden_root():
    return os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "tests", "golden")


def load_dac(args):
    """The DAC arm: --dac_path (DAC.load) or --synthetic dac_* (config of tests/golden/<name>.npz, weights esc.synth.dac_state_dict)."""
    from esc.baselines import DAC
    path, syn = getattr(args, "dac_path", None), getattr(args, "synthetic", None)
    if path:
        dac = DAC.load(path)
    else:
        from esc import synth
        cfg = json.loads(str(np.load(os.path.join(_golden_root(), f"{syn}.npz"))["config_json"]))
        dac = DAC(**cfg)
        man = json.load(open(os.path.join(_golden_root(), f"{syn}_manifest.json")))
        dac.load_state_dict({k: torch.from_numpy(v) for k, v in synth.dac_state_dict(man).items()}, strict=True)
    nq = getattr(args, "n_quantizers", None)
    if isinstance(nq, str):
        nq = [int(v) for v in nq.split(",") if v.strip()]
    return DacEvalModel(dac, nq).eval()


def _is_dac(args):
    return bool(getattr(args, "dac_path", None)) or str(getattr(args, "synthetic", None) or "").startswith("dac_")


def load_model(args):
    if args.model_path:
        cfg = read_yaml(f"{args.model_path}/config.yaml")
        model = make_model(cfg["model"], cfg.get("model_name", "csvq+swinT"))
        model.load_state_dict(torch.load(f"{args.model_path}/model.pth", map_location="cpu")["model_state_dict"])
        return model, cfg["model"]
    from esc import synth
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    g = np.load(os.path.join(root, "tests", "golden", f"{args.synthetic or 'base'}.npz"))
    cfg = json.loads(str(g["config_json"]))
    model = make_model(cfg, str(g["model_name"]) if "model_name" in g else "csvq+swinT")     # csvq+swinT (ESC) or rvq+swinT (RVQCodecs)
    model.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(synth.synth_tensor(k, s))) for k, s in model._state_manifest().items()
                           if not k.endswith(".window")})
    return model, cfg


def _loader(args, model, ragged):
    if ragged:
        return DataLoader(RaggedEvalSet(args.eval_folder_path, model), batch_size=args.batch_size, shuffle=False, collate_fn=ragged_collate)
    return DataLoader(EvalSet(args.eval_folder_path), batch_size=args.batch_size, shuffle=False, collate_fn=default_collate)


def run(args):
    ragged = getattr(args, "ragged", False)
    native = ragged or getattr(args, "native_metrics", False)
    if ragged and getattr(args, "one_pass", False):
        sys.exit("--ragged --one_pass is not implemented: the one-pass sweep takes no per-clip lengths (drop one of the two)")
    if native:
        from esc import metrics as native_metrics
    Mel, Sdr, Counter = (native_metrics.MelSpectrogramDistance, native_metrics.SISDR, native_metrics.EntropyCounter) if native else \
        (MelSpectrogramDistance, SISDR, EntropyCounter)
    metric_funcs = {"MelDistance": Mel().to(args.device), "SISDR": Sdr().to(args.device)}
    try:
        from .metrics import PESQ
        metric_funcs = {"PESQ": PESQ(), **metric_funcs}
    except ImportError:
        print("pesq is not installed: PESQ is skipped", file=sys.stderr)
    epoch = eval_epoch_ragged if ragged else (eval_epoch_one_pass if getattr(args, "one_pass", False) else eval_epoch)
    if _is_dac(args):
        model = load_dac(args).to(args.device)
        eval_loader = _loader(args, model, ragged)
        e_counter = Counter(model.dac.codebook_size, num_streams=model.code_slots(model.max_streams), num_groups=1, device=args.device)
        bps = model.bps_per_stream                  # None: the counts are not k, 2k, ...: the sweep's own lines would carry the wrong kbps
        performances = epoch(model, eval_loader, metric_funcs, e_counter, args.device, num_streams=None, verbose=bps is not None, bps_per_stream=bps or 0.0)
        if bps is None:
            for i in range(model.max_streams):
                line = " | ".join(f"{name}: {vals[i]:.4f}" for name, vals in performances.items())
                print(f"Test Metrics at {model.kbps(i + 1):.2f}kbps ({model.code_slots(i + 1)} codebooks): {line}")
    else:
        model, mcfg = load_model(args)
        model = model.to(args.device)
        eval_loader = _loader(args, model, ragged)
        e_counter = Counter(mcfg["codebook_size"], num_streams=mcfg["max_streams"], num_groups=mcfg["group_size"], device=args.device)
        performances = epoch(model, eval_loader, metric_funcs, e_counter, args.device, num_streams=None, verbose=True, bps_per_stream=1.5)
    save_path = args.save_path or getattr(args, "dac_path", None) and os.path.dirname(args.dac_path) or args.model_path or "."
    os.makedirs(save_path, exist_ok=True)
    json.dump(performances, open(f"{save_path}/perf_stats.json", "w"), indent=2)
    print(f"Test statistics saved into {save_path}/perf_stats.json")
    return performances


if __name__ == "__main__":
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    run(parse_args())
