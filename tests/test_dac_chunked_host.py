"""DAC's chunked compress / decompress (esc.baselines.DAC.compress, DACFile) on the CPU: the delay, get_output_length and the chunk schedule
against the real reference's values (tests/golden/dac_chunk.npz, tools/gen_dac_chunk_golden.py), the DACFile layout and round trip, and the
argument errors that are raised before any device work."""
import numpy as np
import pytest
import torch

import dac_chunk_util as cu
from conftest import load_golden


def _model(name):
    from esc.baselines import DAC
    return DAC(**cu.config_of(load_golden, name))


@pytest.mark.parametrize("name", tuple(cu.GEOMETRY_NS))
def test_delay_and_output_length_are_the_reference(name):
    g = load_golden("dac_chunk")
    m = _model(name)
    assert m.delay == m.get_delay() == int(g[f"{name}_delay"][0])
    for n, want in g[f"{name}_output_length"].tolist():
        assert m.get_output_length(n) == want, n
    base = m.get_output_length(16000)
    for flag in (False, True):                         # neither depends on the padding in effect
        m.padding = flag
        assert m.delay == int(g[f"{name}_delay"][0]) and m.get_output_length(16000) == base
    assert m.padding is True


@pytest.mark.parametrize("case", cu.CASES, ids=[c[0] for c in cu.CASES])
def test_chunk_schedule_is_the_reference(case):
    key, name, win, nt = case
    g = load_golden("dac_chunk")
    delay, hop, n_samples, chunk_length, n_chunks = (int(v) for v in g[f"{key}_geometry"])
    m = _model(name)
    sch = m.chunk_schedule(nt, win)
    assert sch == {"padding": False, "n_samples": n_samples, "hop": hop, "starts": list(range(0, nt, hop)), "chunk_length": chunk_length, "delay": delay}
    assert len(sch["starts"]) == n_chunks and g[f"{key}_codes"].shape[-1] == n_chunks * chunk_length
    assert n_samples - hop != 2 * delay                # the reference's schedule, not a corrected one
    m.padding = False
    assert m.num_frames(n_samples) == chunk_length and m.output_samples(chunk_length) == hop
    m.padding = True
    short = m.chunk_schedule(n_samples, win)           # nt / sr <= win_duration: one padded pass
    assert short["padding"] is True and short["starts"] == [0] and short["hop"] == short["n_samples"] == n_samples
    assert short["chunk_length"] == m.num_frames(n_samples)


def test_unpadded_lengths_and_refusals():
    m = _model("dac_syn")
    m.padding = False
    assert m.num_frames(768) == 128 and m.num_frames(1024) == 192 and m.output_samples(128) == 254
    first = next(n for n in range(1, 2000) if m.num_frames(n) >= 1)
    assert m.num_frames(first - 1) == 0 and m.num_frames(first) == 1 and first > m.hop_length
    tmin = next(t for t in range(1, 500) if m.output_samples(t) >= 1)
    assert m.output_samples(tmin - 1) == 0 and m.output_samples(tmin) >= 1 and tmin > 1
    m.padding = True
    assert m.num_frames(768) == 192 and m.output_samples(192) == 4 * 192     # rates [2, 2]: the padded lengths are back
    with pytest.raises(ValueError):
        m.chunk_schedule(4000, 0.02)                   # 320-sample windows: below the unpadded receptive field


def test_dacfile_round_trip_in_the_reference_layout(tmp_path):
    from esc.baselines import DACFile
    g = load_golden("dac_chunk")
    codes = torch.from_numpy(g["syn1017_codes"].astype(np.int64))
    f = DACFile(codes=codes, chunk_length=128, original_length=1017, input_db=torch.tensor([-23.5]), channels=1, sample_rate=16000, padding=False,
                dac_version="1.0.0")
    path = f.save(tmp_path / "clip.wav")
    assert path.suffix == ".dac"
    raw = np.load(path, allow_pickle=True)[()]         # what the reference's DACFile.load reads (base.py:46-54)
    assert set(raw) == {"codes", "metadata"} and raw["codes"].dtype == np.uint16
    assert set(raw["metadata"]) == {"input_db", "original_length", "sample_rate", "chunk_length", "channels", "padding", "dac_version"}
    assert raw["metadata"]["dac_version"] == "1.0.0" and raw["metadata"]["input_db"].dtype == np.float32
    back = DACFile.load(path)
    assert torch.equal(back.codes, codes) and back.codes.dtype == torch.int64
    assert (back.chunk_length, back.original_length, back.channels, back.sample_rate, back.padding, back.dac_version) == (128, 1017, 1, 16000, False, "1.0.0")
    assert type(back.padding) is bool and float(back.input_db[0]) == -23.5
    raw["metadata"]["dac_version"] = "2.0.0"
    with open(tmp_path / "other.dac", "wb") as fh:
        np.save(fh, raw)
    with pytest.raises(RuntimeError):
        DACFile.load(tmp_path / "other.dac")
    none_db = DACFile(codes=codes, chunk_length=128, original_length=1017, input_db=None, channels=1, sample_rate=16000, padding=False, dac_version="1.0.0")
    assert DACFile.load(none_db.save(tmp_path / "nodb")).input_db is None


def test_argument_errors_without_a_device(tmp_path):
    from esc.baselines import DACFile
    m = _model("dac_syn")
    x = torch.zeros(1, 1, 1017)
    f = DACFile(codes=torch.zeros(1, 4, 128, dtype=torch.int64), chunk_length=128, original_length=500, input_db=None, channels=1, sample_rate=16000,
                padding=True, dac_version="1.0.0")
    with pytest.raises(NotImplementedError):           # training mode (the default after construction), before the device check
        m.compress(x, win_duration=0.048)
    with pytest.raises(NotImplementedError):
        m.decompress(f)
    m.eval()
    with pytest.raises(ValueError, match="sample_rate"):
        m.compress(x, sample_rate=44100, win_duration=0.048)
    f.sample_rate = 44100
    with pytest.raises(ValueError, match="sample_rate"):
        m.decompress(f)
    f.sample_rate = 16000
    with pytest.raises(AssertionError):
        m.padding = 1
    with pytest.raises(AssertionError):
        m.padding = None
    assert m.padding is True
    with pytest.raises(ValueError):
        m.compress(torch.zeros(1, 1, 1, 1017), win_duration=0.048)
    with pytest.raises(ValueError):
        m.compress(x, win_duration=0.048, chunks_per_pass=0)
    m.padding = False
    with pytest.raises(ValueError):                    # too short for the unpadded model: refused on the host, the padding is restored
        m.compress(torch.zeros(1, 1, 4000), win_duration=0.02)
    assert m.padding is False
    with pytest.raises(RuntimeError, match="HIP device"):
        m.compress(x, win_duration=0.048)
    with pytest.raises(RuntimeError, match="HIP device"):
        m.compress(x[..., :768], win_duration=0.048)   # the unchunked pass
    with pytest.raises(RuntimeError, match="HIP device"):
        m.decompress(f)
    assert m.padding is False
