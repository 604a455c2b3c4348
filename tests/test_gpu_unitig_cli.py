"""GPU: the drop-in CLI's --unitigs FILE [--unitigs-min N] [--unitigs-max N] -- the unitigs of the
counted k-mers' de Bruijn graph as FASTA -- against the pure-Python model unitig_model.py on the
counts the same run writes with -a 1."""
import re
import subprocess

import numpy as np
import pytest

from conftest import CLI
import unitig_model as um
from test_gpu_graph_cli import _fasta

pytestmark = pytest.mark.gpu
HEADER = re.compile(r">(\d+) LN:i:(\d+) KC:i:(\d+) km:f:(\d+\.\d)( circular)?$")


def _with_circles(tmp_path):
    """the graph CLI test's reads, and two circles (2 and 60 nodes) read three times round, twice"""
    path = _fasta(tmp_path)
    rng = np.random.default_rng(5)
    c60 = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 60)].tobytes()
    with open(path, "ab") as f:
        for i in range(2):
            f.write(b">ca%d\n%s\n>c60_%d\n%s\n" % (i, b"CA" * 30, i, c60 * 3))
    return path


def _parse(text, k):
    """[(string, n_nodes, count_sum, circular)] of the FASTA, its header fields checked against the strings"""
    lines = text.splitlines()
    assert len(lines) % 2 == 0
    out = []
    for i in range(0, len(lines), 2):
        h = HEADER.match(lines[i])
        assert h, lines[i]
        s = lines[i + 1]
        ln, total = int(h.group(2)), int(h.group(3))
        n = ln - k + 1
        assert int(h.group(1)) == i // 2 and ln == len(s) and n >= 1 and set(s) <= set("ACGT")
        assert h.group(4) == f"{total / n:.1f}"
        out.append((s, n, total, h.group(5) is not None))
    return out


def test_cli_unitigs(tmp_path):
    path, k = _with_circles(tmp_path), 21
    out, u = tmp_path / "out.txt", tmp_path / "unitigs.fa"
    base = [CLI, path, str(k), "-s", "100000"]
    r = subprocess.run(base + ["-a", "1", "-o", str(out), "--unitigs", str(u), "--unitigs-min", "2"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    table = {line.split()[0]: int(line.split()[1]) for line in out.read_text().splitlines()}
    want = um.unitigs(table, 2, 0)
    st = um.stats(want, k)
    assert sorted(x[1] for x in want if x[3]) == [2, 60] and st["unitigs"] > 5 and st["nodes"] > st["unitigs"]
    got = _parse(u.read_text(), k)
    um.check_strings(got, k)
    assert um.normalised(got) == um.normalised(want)
    assert f"Unitigs: {st['unitigs']} ({st['circular']} circular), {st['nodes']} nodes, {st['bases']} bases, " \
           f"longest {st['max_nodes']} nodes" in r.stdout.splitlines()
    # --unitigs-min defaults to the -a value (2); --unitigs-max
    want = um.unitigs(table, 2, 5)
    assert 0 < um.stats(want, k)["nodes"] < st["nodes"]
    r = subprocess.run(base + ["--digest-only", "--unitigs", str(u), "--unitigs-max", "5"], capture_output=True, text=True,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert um.normalised(_parse(u.read_text(), k)) == um.normalised(want)


def test_cli_unitigs_usage_errors(tmp_path):
    path = _fasta(tmp_path)
    out, u = tmp_path / "out.txt", tmp_path / "unitigs.fa"
    base = [CLI, path, "21", "-s", "100000", "-o", str(out)]

    def run(*extra):
        return subprocess.run(base + list(extra), capture_output=True, text=True, cwd=tmp_path)

    for extra in (["--unitigs-min", "2"], ["--unitigs-max", "9"]):
        r = run(*extra)
        assert r.returncode != 0 and "--unitigs-min/--unitigs-max require --unitigs" in r.stderr, extra
    r = run("--unitigs", str(u), "--unitigs-min", "5", "--unitigs-max", "4")
    assert r.returncode != 0 and "minimum above its maximum" in r.stderr
    r = run("--unitigs", str(u), "--unitigs-min", "x")
    assert r.returncode != 0 and "Could not convert" in r.stderr
    assert not out.exists() and not u.exists()  # nothing was counted or written
    assert "--unitigs-min" in subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout
