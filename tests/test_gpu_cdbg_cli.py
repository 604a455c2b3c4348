"""GPU: the drop-in CLI's --gfa FILE [--gfa-min N] [--gfa-max N] -- the compacted de Bruijn graph of
the counted k-mers as GFA 1.0 -- against the pure-Python model cdbg_model.py on the counts the same
run writes with -a 1."""
import re
import subprocess

import pytest

from conftest import CLI
import cdbg_model as cm
import unitig_model as um
from test_gpu_graph_cli import _fasta
from test_gpu_unitig_cli import _with_circles

pytestmark = pytest.mark.gpu
SEGMENT = re.compile(r"S\t(\d+)\t([ACGT]+)\tLN:i:(\d+)\tKC:i:(\d+)$")
LINK = re.compile(r"L\t(\d+)\t([+-])\t(\d+)\t([+-])\t(\d+)M$")


def _parse(text, k):
    """(units, edges, closing) of the GFA: [(string, n_nodes, count_sum, circular)], the edges as the
    model's tuples, and the circles' closing links -- the header first, then the segments in record
    order, then the links; a unitig is circular when it has its two closing links"""
    lines = text.splitlines()
    assert lines[0] == "H\tVN:Z:1.0" and text.endswith("\n")
    segs = [SEGMENT.match(l) for l in lines[1:] if l.startswith("S")]
    links = [LINK.match(l) for l in lines[1 + len(segs):]]
    assert all(segs) and all(links) and len(lines) == 1 + len(segs) + len(links)
    assert [int(s.group(1)) for s in segs] == list(range(len(segs)))
    assert all(int(s.group(3)) == len(s.group(2)) >= k for s in segs) and all(int(l.group(5)) == k - 1 for l in links)
    tuples = [(int(l.group(1)), int(l.group(2) == "-"), int(l.group(3)), int(l.group(4) == "-")) for l in links]
    strings = [s.group(2) for s in segs]
    # a closing link is a self link on one strand whose unitig's last k - 1 bases repeat its first; a
    # homopolymer's loops look the same but its string does not repeat (one node: k bases)
    closing = [t for t in tuples if t[0] == t[2] and t[1] == t[3] and len(strings[t[0]]) > k
               and strings[t[0]][len(strings[t[0]]) - (k - 1):] == strings[t[0]][:k - 1]]
    circular = {t[0] for t in closing}
    assert sorted(closing) == sorted((i, o, i, o) for i in circular for o in (0, 1))
    units = [(s.group(2), len(s.group(2)) - k + 1, int(s.group(4)), i in circular) for i, s in enumerate(segs)]
    edges = [t for t in tuples if t not in closing]
    return units, edges, closing


def test_cli_gfa(tmp_path):
    path, k = _with_circles(tmp_path), 21
    out, gfa = tmp_path / "out.txt", tmp_path / "out.gfa"
    base = [CLI, path, str(k), "-s", "100000"]
    r = subprocess.run(base + ["-a", "1", "-o", str(out), "--gfa", str(gfa), "--gfa-min", "2"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    table = {line.split()[0]: int(line.split()[1]) for line in out.read_text().splitlines()}
    units, edges, st = cm.cdbg(table, 2, 0)
    assert sorted(x[1] for x in units if x[3]) == [2, 60] and st["unitigs"] > 5 and st["edges"] > 0 and st["dead_ends"] > 0
    got_units, got_edges, closing = _parse(gfa.read_text(), k)
    um.check_strings(got_units, k)
    assert um.normalised(got_units) == um.normalised(units) and len(closing) == 2 * st["circular"]
    assert cm.normalised_edges(got_units, got_edges) == cm.normalised_edges(units, edges)
    assert f"Compacted graph: {st['unitigs']} unitigs ({st['circular']} circular), {st['nodes']} nodes, {st['bases']} bases, " \
           f"longest {st['max_nodes']} nodes, {st['edges']} edges, {st['dead_ends']} dead ends" in r.stdout.splitlines()
    # --gfa-min defaults to the -a value (2); --gfa-max
    units, edges, st5 = cm.cdbg(table, 2, 5)
    assert 0 < st5["nodes"] < st["nodes"]
    r = subprocess.run(base + ["--digest-only", "--gfa", str(gfa), "--gfa-max", "5"], capture_output=True, text=True,
                       cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    got_units, got_edges, _ = _parse(gfa.read_text(), k)
    assert um.normalised(got_units) == um.normalised(units)
    assert cm.normalised_edges(got_units, got_edges) == cm.normalised_edges(units, edges)


def test_cli_gfa_usage_errors(tmp_path):
    path = _fasta(tmp_path)
    out, gfa, u = tmp_path / "out.txt", tmp_path / "out.gfa", tmp_path / "unitigs.fa"
    base = [CLI, path, "21", "-s", "100000", "-o", str(out)]

    def run(*extra):
        return subprocess.run(base + list(extra), capture_output=True, text=True, cwd=tmp_path)

    requires = run("--unitigs-min", "2").returncode  # the class of "A requires B"
    for extra in (["--gfa-min", "2"], ["--gfa-max", "9"], ["--unitigs", str(u), "--gfa-min", "2"]):
        r = run(*extra)
        assert r.returncode == requires != 0 and "--gfa-min/--gfa-max require --gfa" in r.stderr, extra
    r = run("--gfa", str(gfa), "--gfa-min", "5", "--gfa-max", "4")
    assert r.returncode != 0 and "minimum above its maximum" in r.stderr
    r = run("--gfa", str(gfa), "--gfa-min", "x")
    assert r.returncode != 0 and "Could not convert" in r.stderr
    assert not out.exists() and not gfa.exists() and not u.exists()  # nothing was counted or written
    assert "--gfa-min" in subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout
