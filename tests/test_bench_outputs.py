"""bench.py's plain line and --dump-outputs: a plain run carries the headline figures and none of
the --full records; the dumped arrays are a function of the output alone (not of the order kc_dump
emits records in), exact in float64, within the size limit, and agree with each other."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, REPO)
BENCH = os.path.join(REPO, "bench.py")


def _records(n, W, seed):
    rng = np.random.default_rng(seed)
    recs = rng.integers(0, 1 << 63, size=(n, W + 1), dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    recs[:, W] = rng.integers(1, 70000, size=n)
    return recs


@pytest.mark.parametrize("W", [1, 2, 4])
@pytest.mark.parametrize("n,cap", [(0, 10), (7, 10), (5000, 5000), (5000, 300)])
def test_sample_is_a_function_of_the_record_set(W, n, cap):
    import bench
    recs = _records(n, W, 100 * W + n)
    a, s = bench.sample_records(recs, 42, cap)
    b, s2 = bench.sample_records(recs[np.random.default_rng(1).permutation(n)], 42, cap)
    assert s == s2 and np.array_equal(a, b)
    assert a.shape[0] <= cap and (s == 0) == (n <= 0.8 * cap)
    if s == 0:
        assert a.shape[0] == n
    else:  # about n / 2^s records, every one of them a record of the input
        assert 0.5 * n / 2**s < a.shape[0] < 1.5 * n / 2**s
        assert {r.tobytes() for r in a} <= {r.tobytes() for r in recs}
    keys = [tuple(int(x) for x in r[:W]) for r in a]
    assert keys == sorted(keys)
    if n > 300:  # another seed, another sample
        c, _ = bench.sample_records(recs, 43, 300)
        d, _ = bench.sample_records(recs, 42, 300)
        assert not np.array_equal(c, d)


def test_key_words_survive_float64_as_halves():
    import bench
    a = np.array([[0, 1, 2**32 - 1, 2**32, 2**53 + 1, 2**64 - 1]], dtype=np.uint64)
    h = bench._halves(a)
    assert h.dtype == np.float64 and h.shape == (1, 12)
    back = [(int(h[0, 2 * i]) << 32) | int(h[0, 2 * i + 1]) for i in range(6)]
    assert back == [int(x) for x in a[0]]


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_plain_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--reads", "20000",
                        "--genome", "100000", "--slots", "4000000", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=280)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "k-mers/s" and d["dtype"] == "u64"
    assert d["higher_is_better"] is True and d["ms_per_step"] > 0
    windows = 20000 * (150 - 31 + 1)
    assert d["windows_per_step_per_gpu"] == windows
    assert d["value"] == pytest.approx(windows / (d["ms_per_step"] * 1e-3), rel=1e-9)
    # none of the records that take runs of their own
    for key in ("c3", "c4", "c5", "parity", "writer", "compact", "cli_fullsize", "c_abi_host_chunks"):
        assert key not in d, key
    assert d["cpu_baseline"] is None

    files = {f: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(files) == {"stats.npy", "digest.npy", "keys.npy", "counts.npy", "sample.npy"}
    assert all(a.dtype == np.float64 for a in files.values())
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    stats, dig, keys, counts, sample = (files[n + ".npy"] for n in ("stats", "digest", "keys", "counts", "sample"))
    assert stats[0] == windows and stats[2] == d["distinct_per_gpu"]
    # this small output is dumped whole: the records are the digest's lines, sorted by key, and
    # their counts add up to the digest's
    assert sample[1] == 0 and sample[0] == sample[2] == keys.shape[0] == counts.shape[0] == dig[0]
    assert 0 < dig[0] <= stats[2] and counts.min() >= 1 and counts.sum() == dig[1]
    assert keys.shape[1] == 2 and keys.max() < 2**32
    k64 = keys[:, 0].astype(np.uint64) * np.uint64(2**32) + keys[:, 1].astype(np.uint64)
    assert np.all(k64[1:] > k64[:-1])
