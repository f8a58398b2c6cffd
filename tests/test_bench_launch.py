"""bench.py's launcher: `--gpus N` starts its own N ranks, refuses a node with fewer devices, defaults to the fixed
288-clip job of BASELINE configs[3] for N > 1 and to configs[1] (36 clips) for N = 1, and reports `n_gpus` from the communicator.
CPU part: the dry-run mode (gloo ranks, no model) runs the real launcher + job resolution + shard plan + code all-gather.  GPU part: the
refusal on a 1-GPU box and a self-launched one-rank run whose exchange step goes through RCCL and the C-ABI collective."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
BENCH = os.path.join(ROOT, "bench.py")


def _run(args, env=None, timeout=600):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=e, timeout=timeout)


def _json_line(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


def test_job_resolution_and_launcher_command():
    import bench
    assert bench.resolve_job(1) == (False, 36)                          # BASELINE configs[1]
    for n in (2, 4, 8):
        assert bench.resolve_job(n) == (True, 288)                      # BASELINE configs[3]: fixed job, strong scaling
        assert bench.resolve_job(n, weak=True) == (False, 36 * n)
    assert bench.resolve_job(1, global_batch=288) == (True, 288)
    assert bench.resolve_job(3, global_batch=100) == (True, 100)
    with pytest.raises(SystemExit):
        bench.resolve_job(2, global_batch=288, weak=True)
    cmd = bench.launcher_command(["--gpus", "4", "--steps", "3"], 4, 29999)
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and "--nproc-per-node=4" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29999"
    assert cmd[-5:] == [BENCH, "--gpus", "4", "--steps", "3"]


@pytest.mark.parametrize("n,extra,scaling,total,per_rank", [(2, [], "strong", 288, [144, 144]), (3, ["--weak"], "weak", 108, [36, 36, 36]),
                                                            (3, ["--global-batch", "100"], "strong", 100, [34, 33, 33])])
def test_self_launch_runs_n_ranks_and_reports_the_communicator(n, extra, scaling, total, per_rank):
    r = _run(["--gpus", str(n), "--dry-run"] + extra)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == n and d["scaling"] == scaling and d["config"]["global_batch"] == total and d["config"]["clips_per_rank"] == per_rank
    if scaling == "strong" and total == 288:
        assert "configs[3]" in d["config"]["workload"]
    assert "torch.distributed.run" in r.stderr                           # it went through the launcher, not one process pretending


def test_one_gpu_default_is_the_quoted_configuration():
    d = _json_line(_run(["--dry-run"]).stdout)
    assert d["n_gpus"] == 1 and d["scaling"] == "weak" and d["config"]["global_batch"] == 36 and "configs[1]" in d["config"]["workload"]


def test_flag_and_launcher_must_agree():
    r = _run(["--gpus", "1", "--dry-run"], env={"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode != 0 and "disagree" in r.stderr


@pytest.mark.skipif(__import__("torch").cuda.is_available(), reason="needs a node WITHOUT devices (the GPU variant is below)")
def test_refuses_more_gpus_than_the_node_has_cpu():
    r = _run(["--gpus", "2"])
    assert r.returncode != 0 and "refusing" in r.stderr and not [l for l in r.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_refuses_more_gpus_than_the_node_has():
    import torch
    n = torch.cuda.device_count() + 1
    r = _run(["--gpus", str(n)])
    assert r.returncode != 0 and "refusing" in r.stderr and not [l for l in r.stdout.splitlines() if l.startswith("{")]


@pytest.mark.gpu
def test_self_launched_rank_gathers_through_rccl_and_the_c_abi():
    """One rank (this box has one GPU) launched BY bench.py under torch.distributed.run, process group on RCCL, the code exchange through
    escx_allgather_codes on a communicator created by esc.distributed.AbiCodesGather; then the same through torch.distributed."""
    for abi in ("1", "0"):
        r = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--skip-isolated", "--skip-single-clip", "--profile-steps", "1"],
                 env={"ESCX_BENCH_SELF_LAUNCH": "1", "ESCX_BENCH_FORCE_DIST": "1", "ESCX_BENCH_ABI_COLLECTIVE": abi})
        assert r.returncode == 0, r.stderr[-3000:]
        d = _json_line(r.stdout)
        assert d["n_gpus"] == 1 and d["value"] > 1000 and "torch.distributed.run" in r.stderr
        assert ("escx_allgather_codes C ABI" if abi == "1" else "torch.distributed") in d["config"]["parallelism"]


@pytest.mark.gpu
def test_data_parallel_training_step_touches_rccl():
    """bench.py --mode train with a forced one-rank RCCL group: the flat-gradient all-reduce (esc.distributed.all_reduce_gradients) runs on
    the device through `nccl` (VERDICT r2 missing #3) and the step still trains."""
    r = _run(["--mode", "train", "--gpus", "1", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"], env={"ESCX_BENCH_FORCE_DIST": "1"})
    assert r.returncode == 0, r.stderr[-3000:]
    d = _json_line(r.stdout)
    assert d["n_gpus"] == 1 and "all-reduce over RCCL" in d["config"]["parallelism"] and d["value"] > 100


def test_plain_run_is_lean_and_full_is_an_option():
    """`--full` carries the extras (profile passes, CPU baseline, riders); `--dump-outputs DIR` exists; `--steps` is the count of timed steps."""
    r = _run(["--help"])
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = _run(["--steps", "0"])
    assert r.returncode != 0 and "--steps" in r.stderr


def test_dump_outputs_writes_fixed_float_arrays(tmp_path):
    import numpy as np
    import torch
    import bench
    codes = torch.arange(36 * 6 * 3 * 5, dtype=torch.int64).view(36, 6, 3, 5) % 1024
    audio = torch.linspace(-1, 1, 36 * 480).view(36, 480)
    big = torch.arange(bench.DUMP_SAMPLE + 1000, dtype=torch.float32)
    for d in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(str(d), {"codes": codes, "audio": audio, "big": big, "half": audio.bfloat16()})
    a = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in ("codes", "audio", "big", "half")}
    assert a["codes"].dtype == np.float64 and np.array_equal(a["codes"], codes.numpy())
    assert a["audio"].dtype == np.float32 and np.array_equal(a["audio"], audio.numpy())
    assert a["half"].dtype == np.float32 and a["half"].shape == (36, 480)
    assert a["big"].shape == (bench.DUMP_SAMPLE,) and np.all(np.diff(a["big"]) > 0)          # sorted sample of the flat elements
    assert np.array_equal(a["big"], np.load(tmp_path / "b" / "big.npy"))                       # the same sample in every run
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "c"), {f"x{i}": big for i in range(5)})             # 5 x 16 MB > 64 MB
