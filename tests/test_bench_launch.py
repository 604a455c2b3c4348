"""bench.py's multi-rank launch: `python bench.py --gpus N` without a
launcher starts N rank processes itself, and a WORLD_SIZE that disagrees with --gpus is an
error, never a silent one-GPU run.  CPU only: --launch-only joins a gloo process group and
reports the ranks that joined, without any GPU work."""
import json
import os
import subprocess
import sys

import pytest

from conftest import REPO

BENCH = os.path.join(REPO, "bench.py")


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env.update(extra)
    return env


def _json_line(out):
    lines = [ln for ln in out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out
    return json.loads(lines[0])


@pytest.mark.parametrize("n", [2, 3])
def test_gpus_n_spawns_n_ranks(n):
    p = subprocess.run([sys.executable, BENCH, "--gpus", str(n), "--launch-only", "--backend", "gloo"],
                       capture_output=True, text=True, timeout=180, env=_env())
    assert p.returncode == 0, p.stderr[-2000:]
    d = _json_line(p.stdout)
    assert d["n_gpus"] == n and d["ranks_joined"] == n


def test_world_size_mismatch_is_refused():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2"], capture_output=True, text=True, timeout=120,
                       env=_env(WORLD_SIZE="3", RANK="0"))
    assert p.returncode != 0
    assert "WORLD_SIZE=3" in p.stderr
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


def test_gpus_beyond_visible_devices_is_refused():
    """On a host without enough GPUs the launcher refuses instead of timing fewer ranks, and it
    counts them without importing torch (VERDICT r4 item 1 / ADVICE r4: no HIP call in the parent
    of the ranks)."""
    code = ("import runpy, sys\nsys.argv = [%r, '--gpus', '2']\ntry:\n    runpy.run_path(%r, run_name='__main__')\n"
            "except SystemExit as e:\n    print('EXIT', e.code, 'torch' in sys.modules)\n") % (BENCH, BENCH)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120,
                       env=_env(HIP_VISIBLE_DEVICES="0"))
    assert "EXIT 2 False" in p.stdout, p.stdout + p.stderr
    assert "GPU(s) visible" in p.stderr


def test_visible_gpus_reads_the_device_lists(monkeypatch):
    import bench
    for var in ("ROCR_VISIBLE_DEVICES", "HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setenv("ROCR_VISIBLE_DEVICES", "0,1,2")
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "0,1")
    n = bench.visible_gpus()
    assert n is not None and n <= 2


@pytest.mark.gpu
def test_gpus_two_on_a_one_gpu_box_fails_without_a_line():
    """The one-GPU box: --gpus 2 must not produce a bench line (the launcher refuses with exit 2
    when sysfs shows one GPU; else a rank fails at set_device)."""
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "1", "--warmup", "0"], capture_output=True,
                       text=True, timeout=300, env=_env())
    assert p.returncode != 0
    assert not [ln for ln in p.stdout.splitlines() if ln.startswith("{")]


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_two_rank_line_rehearsed_on_one_gpu_matches_one_gpu():
    """The N > 1 line's code path end to end (--rehearse-one-gpu: two ranks on cuda:0 over gloo):
    the default strong C4 line at a small read count with its c2 record and xgmi record, whose
    combined owner digest equals the same job's on one GPU."""
    common = ["--full", "--reads", "200000", "--steps", "1", "--warmup", "0", "--no-cpu-baseline", "--no-compact",
              "--no-writer", "--no-cli-fullsize"]
    p2 = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rehearse-one-gpu"] + common, capture_output=True,
                        text=True, timeout=500, env=_env())
    assert p2.returncode == 0, p2.stderr[-3000:]
    d2 = _json_line(p2.stdout)
    assert d2["n_gpus"] == 2 and d2["scaling"] == "strong" and d2["config"]["workload"].startswith("C4")
    assert "xgmi" in d2 and d2["xgmi"]["sent_bytes_per_step_per_rank"] > 0 and "c2" in d2
    # (the strong line takes the super-k-mer exchange: bytes per window sent and the G = 2/4/8 model)
    assert d2["xgmi"]["exchange"] == "superkmers" and set(d2["xgmi"]["model_sent_bytes_per_rank"]) == {"2", "4", "8"}
    assert 0.2 < d2["xgmi"]["bytes_per_window_sent"] < 3.0
    p1 = subprocess.run([sys.executable, BENCH, "--config", "C4"] + common, capture_output=True, text=True,
                        timeout=300, env=_env())
    assert p1.returncode == 0, p1.stderr[-3000:]
    d1 = _json_line(p1.stdout)
    assert d2["parity"]["digest"] == d1["parity"]["digest"]
    assert d2["windows_per_step_per_gpu"] * 2 == d1["windows_per_step_per_gpu"]
