"""GPU: the drop-in CLI's table operations -- --op NAME --with FILE2 [--a-min/--a-max/--b-min/--b-max N]
-- against the model (tableop_model.py) applied to the C oracle's counts of the two files."""
import subprocess

import numpy as np
import pytest

from conftest import CLI, lines_digest, oracle_count
import tableop_model as m

pytestmark = pytest.mark.gpu

K = 31


def _fasta(rng, genome, n, length):
    starts = rng.integers(0, len(genome) - length + 1, n)
    return "".join(f">r{i}\n{genome[s:s + length]}\n" for i, s in enumerate(starts))


@pytest.fixture(scope="module")
def two_files(tmp_path_factory):
    """two small FASTA files whose genomes share half their sequence, and the oracle's raw counts"""
    d = tmp_path_factory.mktemp("tableop_cli")
    rng = np.random.default_rng(8)
    shared, own_a, own_b = ("".join(rng.choice(list("ACGT"), size=5000)) for _ in range(3))
    tables = []
    for name, genome in (("a.fasta", shared + own_a), ("b.fasta", shared + own_b)):
        (d / name).write_text(_fasta(rng, genome, 600, 100))
        exp = d / (name + ".oracle")
        oracle_count(str(d / name), K, ["-m", "2", "-a", "1"], exp)
        with open(exp) as f:
            tables.append({s: int(c) for s, c in (line.split() for line in f)})
    assert max(max(t.values()) for t in tables) < 16383  # raw count = T(c)
    return d, tables[0], tables[1]


def _lines(raw, a):
    return sorted(f"{s} {c}\n" for s, c in m.read_back(raw, 2, min_abundance=a).items())


def test_cli_subtract(two_files, tmp_path):
    d, ta, tb = two_files
    out = tmp_path / "child_only.txt"
    r = subprocess.run([CLI, str(d / "a.fasta"), str(K), "-a", "2", "-s", "100000", "-o", str(out), "--op", "subtract",
                        "--with", str(d / "b.fasta")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw, st = m.table_op(ta, tb, m.OP_SUBTRACT)
    want = _lines(raw, 2)
    assert 100 < len(want) < len(raw)
    assert sorted(out.read_text().splitlines(keepends=True)) == want
    assert f"Table operation subtract with b.fasta: {st['a_keys']} k-mers of the input in range, {st['both']} of them" in r.stdout


@pytest.mark.parametrize("name,extra,ranges", [
    ("union-sum", [], {}),
    ("intersect-min", ["--a-min", "2", "--b-max", "3"], dict(a_range=(2, 0), b_range=(0, 3))),
    ("counts-subtract", ["--b-min=2"], dict(b_range=(2, 0))),
])
def test_cli_ops_ranges_histo_and_digest(name, extra, ranges, two_files, tmp_path):
    d, ta, tb = two_files
    raw, _ = m.table_op(ta, tb, m.OP_NAMES.index(name), **ranges)
    out, h = tmp_path / "out.txt", tmp_path / "h.txt"
    base = [CLI, str(d / "a.fasta"), str(K), "-a", "1", "-s", "100000", "--op", name, "--with", str(d / "b.fasta")] + extra
    r = subprocess.run(base + ["-o", str(out), "--histo", str(h)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert sorted(out.read_text().splitlines(keepends=True)) == _lines(raw, 1)
    spectrum = np.bincount(np.array(list(raw.values()), dtype=np.int64))
    assert h.read_text() == "".join(f"{v} {n}\n" for v, n in enumerate(spectrum.tolist()) if n)
    r = subprocess.run(base + ["--digest-only"], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    dg = lines_digest(_lines(raw, 1))
    assert f'"lines": {dg["lines"]}, "count_sum": {dg["count_sum"]}, "hash_sum": "{dg["hash_sum"]}"' in r.stdout


def test_cli_table_op_usage_errors(two_files, tmp_path):
    d, _, _ = two_files
    a, b, out = str(d / "a.fasta"), str(d / "b.fasta"), tmp_path / "out.txt"
    for args, msg in ((["--op", "subtract"], "--op requires --with"),
                      (["--with", b], "--with requires --op"),
                      (["--op", "minus", "--with", b], "--op: Value minus not in"),
                      (["--op", "subtract", "--with", str(tmp_path / "missing.fasta")], "--with: File does not exist"),
                      (["--a-min", "2"], "require --op"),
                      (["--op", "subtract", "--with", b, "--a-min", "3", "--a-max", "2"], "minimum above its maximum")):
        r = subprocess.run([CLI, a, str(K), "-s", "100000", "-o", str(out)] + args, capture_output=True, text=True,
                           cwd=tmp_path)
        assert r.returncode != 0, args
        assert msg in r.stderr, (args, r.stderr)
        assert not out.exists() and not list(tmp_path.glob("*.kaarme_counts"))
