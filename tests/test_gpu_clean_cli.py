"""GPU: the drop-in CLI's graph cleaning -- --clean-tips N, --clean-isolated N, --clean-max-mean M,
--clean-rounds R, --clean-min/--clean-max N, --clean-out FILE, --clean-stats FILE -- against the
pure-Python model clean_model.py on the counts the same run writes with -a 1: --gfa then reads the
cleaned table, -o still the counted one."""
import subprocess

import pytest

from conftest import CLI
import cdbg_model as cm
import clean_cases as cc
import clean_model as clm
import unitig_model as um
from test_gpu_cdbg_cli import _parse
from test_gpu_graph_cli import _fasta
from test_gpu_unitig_cli import _with_circles

pytestmark = pytest.mark.gpu


def _input(tmp_path, k):
    """the unitig CLI test's reads and circles (forks and bubbles, but hardly a tip) and, each twice, the
    cascade of clean_cases (three tips of k - 1 nodes, one of them only a tip once the others are gone)
    and a 10-node chain beside its genome"""
    path = _with_circles(tmp_path)
    with open(path, "ab") as f:
        f.write(cc.fasta((cc.cascade(k, n=k - 1)[0] + cc.isolated_chain(k, n=10)[0]) * 2))
    return path


def _table(path):
    return {line.split()[0]: int(line.split()[1]) for line in path.read_text().splitlines()}


def _stats_lines(path):
    """[{name: value}] of the --clean-stats file, a line of "name value" pairs per round"""
    out = []
    for line in path.read_text().splitlines():
        f = line.split()
        assert len(f) % 2 == 0
        out.append({f[i]: int(f[i + 1]) for i in range(0, len(f), 2)})
    return out


def test_cli_clean(tmp_path):
    k = 21
    path = _input(tmp_path, k)
    out, gfa, cout, cst = tmp_path / "out.txt", tmp_path / "out.gfa", tmp_path / "clean.txt", tmp_path / "clean.stats"
    base = [CLI, path, str(k), "-s", "100000", "-a", "1"]
    clean = ["--clean-tips", str(k - 1), "--clean-isolated", str(k - 1), "--clean-rounds", "10", "--clean-min", "2"]
    r = subprocess.run(base + ["-o", str(out), "--gfa", str(gfa)] + clean + ["--clean-out", str(cout), "--clean-stats", str(cst)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    table = _table(out)
    rule = dict(min_count=2, tip_max_nodes=k - 1, iso_max_nodes=k - 1)
    want, want_st = clm.model_rounds(table, 10, **rule)
    # the input has what the options are for, the rounds end early, and the circles stay
    assert [(st["tips"], st["isolated"]) for st in want_st] == [(2, 1), (1, 0), (0, 0)] and 0 < len(want) < len(table)
    # --clean-stats: one line per round run
    assert _stats_lines(cst) == [dict(st, round=i + 1) for i, st in enumerate(want_st)]
    assert r.stdout.count("Graph cleaning round ") == len(want_st)
    # --clean-out: every k-mer of the cleaned table, as -o writes them
    assert _table(cout) == want and cout.read_text().endswith("\n")
    assert sorted(cout.read_text().splitlines()) == sorted(f"{c} {t}" for c, t in want.items())
    # --gfa reads the cleaned table, with its own range (the -a value: 1) applied to it
    units, edges, st = cm.cdbg(want, 1, 0)
    assert sorted(x[1] for x in units if x[3]) == [2, 60] and st["edges"] > 0
    got_units, got_edges, closing = _parse(gfa.read_text(), k)
    um.check_strings(got_units, k)
    assert um.normalised(got_units) == um.normalised(units) and len(closing) == 2 * st["circular"]
    assert cm.normalised_edges(got_units, got_edges) == cm.normalised_edges(units, edges)
    assert cm.normalised_edges(got_units, got_edges) != cm.normalised_edges(*cm.cdbg(table, 2, 0)[:2])
    # -o still reads the counted table: the same file with and without the clean options.  Two runs of
    # the CLI write their lines in different orders, clean options or not (kc_write's line order is
    # unspecified: a slot's place in its bucket is settled by a race of the counting pass), so the
    # files are compared as their sorted lines and their sizes, not byte by byte.
    plain = tmp_path / "plain.txt"
    r = subprocess.run(base + ["-o", str(plain)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert sorted(plain.read_bytes().split(b"\n")) == sorted(out.read_bytes().split(b"\n"))
    assert len(plain.read_bytes()) == len(out.read_bytes()) > 0
    # one rule alone, one round, the default range (the -a value: 1); --gfa-min on the cleaned table
    r = subprocess.run(base + ["--digest-only", "--gfa", str(gfa), "--gfa-min", "2", "--clean-tips", str(k - 1),
                               "--clean-stats", str(cst)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    want1, st1 = clm.clean(table, 1, 0, tip_max_nodes=k - 1)
    assert st1["tips"] == 3 and st1["isolated"] == 0 and _stats_lines(cst) == [dict(st1, round=1)]
    units, edges, st = cm.cdbg(want1, 2, 0)
    got_units, got_edges, _ = _parse(gfa.read_text(), k)
    assert um.normalised(got_units) == um.normalised(units)
    assert cm.normalised_edges(got_units, got_edges) == cm.normalised_edges(units, edges)
    # the guard: no tip here has a mean count of 1, so --clean-max-mean 1 keeps them all
    r = subprocess.run(base + ["--digest-only", "--clean-tips", str(k - 1), "--clean-max-mean", "1", "--clean-stats", str(cst)],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    st0 = clm.clean(table, 1, 0, tip_max_nodes=k - 1, max_mean=1)[1]
    assert st0["tips"] == 0 and _stats_lines(cst) == [dict(st0, round=1)]


def test_cli_clean_usage_errors(tmp_path):
    path = _fasta(tmp_path)
    out, gfa, f = tmp_path / "out.txt", tmp_path / "out.gfa", tmp_path / "clean.txt"
    base = [CLI, path, "21", "-s", "100000", "-o", str(out)]

    def run(*extra):
        return subprocess.run(base + list(extra), capture_output=True, text=True, cwd=tmp_path)

    requires = run("--gfa-min", "2").returncode  # the class of "A requires B"
    for extra in (["--clean-max-mean", "5"], ["--clean-rounds", "2"], ["--clean-min", "2"], ["--clean-max", "9"],
                  ["--clean-out", str(f)], ["--clean-stats", str(f)], ["--gfa", str(gfa), "--clean-rounds", "3"]):
        r = run(*extra)
        assert r.returncode == requires != 0 and "require --clean-tips or --clean-isolated" in r.stderr, extra
    r = run("--clean-tips", "20", "--clean-min", "5", "--clean-max", "4")
    assert r.returncode != 0 and "minimum above its maximum" in r.stderr
    for opt in ("--clean-tips", "--clean-isolated", "--clean-max-mean", "--clean-rounds", "--clean-min", "--clean-max"):
        r = run("--clean-isolated", "20", opt, "x")
        assert r.returncode != 0 and "Could not convert" in r.stderr, opt
    r = run("--clean-tips", "20", "--clean-rounds", "0")
    assert r.returncode != 0 and "--clean-rounds" in r.stderr
    r = run("--clean-tips", "20", "--op", "union-sum", "--with", path)
    assert r.returncode != 0 and "exclude --op" in r.stderr
    assert not out.exists() and not gfa.exists() and not f.exists()  # nothing was counted or written
    assert "--clean-tips" in subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout
