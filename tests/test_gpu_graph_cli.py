"""GPU: the drop-in CLI's --graph FILE [--graph-min N] [--graph-max N] [--graph-stats FILE] -- a
line per node of the counted k-mers' de Bruijn graph, and the graph's statistics -- against the
pure-Python model graph_model.py on the counts the same run writes with -a 1."""
import subprocess

import numpy as np
import pytest

from conftest import CLI
import graph_model as m

pytestmark = pytest.mark.gpu


def _fasta(tmp_path):
    rng = np.random.default_rng(3)
    genome = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 3000)].tobytes()
    genome = genome[:1500] + genome[200:400] + genome[1500:]  # a 200-base repeat: forks
    path = tmp_path / "reads.fasta"
    with open(path, "wb") as f:
        for i, s in enumerate(rng.integers(0, len(genome) - 80, 300)):
            r = bytearray(genome[s:s + 80])
            if i % 7 == 0:
                r[40] = b"ACGT"[(b"ACGT".index(r[40]) + 1) % 4]  # tips and bubbles
            f.write(b">r%d\n%s\n" % (i, bytes(r)))
    return str(path)


def _stats_lines(st):
    return [f"{n} {st[n]}" for n in m.FIELDS] + [f"side_degree_{d} {v}" for d, v in enumerate(st["side_degree"])] + \
           [f"open_unitigs {st['open_unitigs']}"]


def test_cli_graph(tmp_path):
    path, k = _fasta(tmp_path), 21
    out, g, gs = tmp_path / "out.txt", tmp_path / "graph.txt", tmp_path / "graph_stats.txt"
    base = [CLI, path, str(k), "-s", "100000"]
    # next to the counting run and its output file; -a 1: every k-mer is written and is a node
    r = subprocess.run(base + ["-a", "1", "-o", str(out), "--graph", str(g), "--graph-stats", str(gs)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    table = {line.split()[0]: int(line.split()[1]) for line in out.read_text().splitlines()}
    assert len(table) > 3000
    flags, st = m.graph(table)
    assert st["side_degree"][0] > 0 and st["side_degree"][2] > 0 and st["link_ends"] > 100
    assert sorted(g.read_text().splitlines()) == sorted(m.node_line(c, table[c], f) for c, f in flags.items())
    assert gs.read_text().splitlines() == _stats_lines(st)
    assert f"De Bruijn graph: {st['nodes']} nodes, {st['edge_ends']} edge ends, {st['link_ends']} link ends, " \
           f"{st['open_unitigs']} open unitigs" in r.stdout.splitlines()
    # --graph-min defaults to the -a value; --graph-max
    flags, st = m.graph(table, 2, 5)
    assert 100 < st["nodes"] < len(table)
    r = subprocess.run(base + ["--digest-only", "--graph", str(g), "--graph-max", "5", "--graph-stats", str(gs)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert sorted(g.read_text().splitlines()) == sorted(m.node_line(c, table[c], f) for c, f in flags.items())
    assert gs.read_text().splitlines() == _stats_lines(st)
    # --graph-stats alone, and an explicit --graph-min without --graph-stats
    g.unlink()
    r = subprocess.run(base + ["--digest-only", "--graph-stats", str(gs)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert gs.read_text().splitlines() == _stats_lines(m.graph(table, 2, 0)[1]) and not g.exists()
    flags, st = m.graph(table, 3, 0)
    r = subprocess.run(base + ["--digest-only", "--graph", str(g), "--graph-min", "3"], capture_output=True, text=True,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert sorted(g.read_text().splitlines()) == sorted(m.node_line(c, table[c], f) for c, f in flags.items())


def test_cli_graph_usage_errors(tmp_path):
    path = _fasta(tmp_path)
    out, g, gs = tmp_path / "out.txt", tmp_path / "graph.txt", tmp_path / "graph_stats.txt"
    base = [CLI, path, "21", "-s", "100000", "-o", str(out)]

    def run(*extra):
        return subprocess.run(base + list(extra), capture_output=True, text=True, cwd=tmp_path)

    for extra in (["--graph-min", "2"], ["--graph-max", "9"], ["--graph-min", "2", "--graph-stats", str(gs)],
                  ["--graph-max", "9", "--graph-stats", str(gs)]):
        r = run(*extra)
        assert r.returncode != 0 and "--graph-min/--graph-max require --graph" in r.stderr, extra
    r = run("--graph", str(g), "--graph-min", "5", "--graph-max", "4")
    assert r.returncode != 0 and "minimum above its maximum" in r.stderr
    r = run("--graph", str(g), "--graph-min", "x")
    assert r.returncode != 0 and "Could not convert" in r.stderr
    r = run("--graph")
    assert r.returncode != 0
    assert not out.exists() and not g.exists() and not gs.exists()  # nothing was counted or written
    assert "--graph-stats" in subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout
