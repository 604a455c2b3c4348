"""GPU: the drop-in CLI's weak-link removal -- --cut-weak N, --cut-ratio P, --cut-max-mean M,
--cut-rounds R, --cut-min/--cut-max N, --cut-out FILE, --cut-stats FILE -- against the pure-Python
model weak_model.py on the counts the same run writes with -a 1: --gfa then reads the cut table, -o
still the counted one, and with --clean-* and --pop-* those rounds run first."""
import subprocess

import numpy as np
import pytest

from conftest import CLI
import bubble_cases as bc
import bubble_model as bm
import cdbg_model as cm
import clean_cases as cc
import clean_model as clm
import unitig_model as um
import weak_cases as wc
import weak_model as wm
from test_gpu_cdbg_cli import _parse
from test_gpu_clean_cli import _stats_lines, _table
from test_gpu_graph_cli import _fasta

pytestmark = pytest.mark.gpu


def _run(args, cwd):
    r = subprocess.run(args, capture_output=True, text=True, cwd=cwd)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_cut_weak_to_two_segments(tmp_path):
    k = 31
    seqs, j = wc.chimera(k)
    path = tmp_path / "chimera.fasta"
    path.write_bytes(cc.fasta(seqs))
    out, gfa, wout, wst = tmp_path / "out.txt", tmp_path / "out.gfa", tmp_path / "cut.txt", tmp_path / "cut.stats"
    base = [CLI, str(path), str(k), "-s", "100000", "-a", "1"]
    _run(base + ["-o", str(out), "--gfa", str(gfa)], tmp_path)
    units, edges, _ = _parse(gfa.read_text(), k)
    assert len(units) == 5 and len(edges) == 8  # without the option the joint ties G1 to G2
    r = _run(base + ["-o", str(out), "--gfa", str(gfa), "--cut-weak", str(k), "--cut-out", str(wout), "--cut-stats", str(wst)],
             tmp_path)
    table = _table(out)
    want, want_st = wm.cut(table, max_nodes=k, ratio_permille=200)  # --cut-ratio defaults to 200
    assert want_st["cut"] == 1 and len(want) == 200 == len(table) - (k - 1)
    assert _stats_lines(wst) == [dict(want_st, round=1)] and r.stdout.count("Weak-link removal round ") == 1
    assert _table(wout) == want and sorted(wout.read_text().splitlines()) == sorted(f"{c} {t}" for c, t in want.items())
    got_units, got_edges, closing = _parse(gfa.read_text(), k)
    assert sorted(u[1] for u in got_units) == [100, 100] and not got_edges and not closing
    assert um.normalised(got_units) == um.normalised(cm.cdbg(want)[0])
    # the ratio, the guard and the range in one more run: no relative test, the guard alone decides
    _run(base + ["--digest-only", "--cut-weak", str(k), "--cut-ratio", "0", "--cut-max-mean", "1", "--cut-max", "10",
                 "--cut-stats", str(wst)], tmp_path)
    st = wm.cut(table, 1, 10, max_nodes=k, max_mean=1)[1]
    assert st["cut"] == 1 and _stats_lines(wst) == [dict(st, round=1)]


def test_cli_cut_rounds_after_clean_and_pop(tmp_path):
    """the chimera, a substituted variant of G1 and a tip off G2, once each: the cut rounds run on the
    table that the cleaning and then the popping left"""
    k = 21
    seqs, j = wc.chimera(k)
    g1, g2 = seqs[0], seqs[10]
    variant = bc.substituted(g1, 45, k, 1)
    tip = cc.branch(np.random.default_rng(4), g2, 70, 4, k)
    path = tmp_path / "chain.fasta"
    path.write_bytes(cc.fasta(seqs + [variant, tip]))
    out, gfa = tmp_path / "out.txt", tmp_path / "out.gfa"
    cst, pst, wst = tmp_path / "clean.stats", tmp_path / "pop.stats", tmp_path / "cut.stats"
    base = [CLI, str(path), str(k), "-s", "100000", "-a", "1", "-o", str(out)]
    cut = ["--cut-weak", str(2 * k), "--cut-ratio", "300", "--cut-rounds", "5", "--cut-stats", str(wst)]
    # cutting alone: the variant's arm is a weak link too, and the tip stays
    _run(base + cut + ["--gfa", str(gfa)], tmp_path)
    table = _table(out)
    rule = dict(max_nodes=2 * k, ratio_permille=300)
    want, want_st = wm.model_rounds(table, 5, **rule)
    assert [s["cut"] for s in want_st] == [2, 0]
    assert _stats_lines(wst) == [dict(st, round=i + 1) for i, st in enumerate(want_st)]
    units, edges, _ = cm.cdbg(want)
    got_units, got_edges, _ = _parse(gfa.read_text(), k)
    assert um.normalised(got_units) == um.normalised(units) and len(units) == 4
    assert cm.normalised_edges(got_units, got_edges) == cm.normalised_edges(units, edges)
    # cleaning, popping, then cutting: G1 and G2
    r = _run(base + ["--clean-tips", str(k - 1), "--clean-stats", str(cst), "--pop-bubbles", str(k), "--pop-stats", str(pst)]
             + cut + ["--gfa", str(gfa)], tmp_path)
    cleaned, clean_st = clm.clean(table, 1, 0, tip_max_nodes=k - 1)
    popped, pop_st = bm.pop(cleaned, 1, 0, max_nodes=k)
    assert clean_st["tips"] == 1 and pop_st["popped"] == 1
    assert _stats_lines(cst) == [dict(clean_st, round=1)] and _stats_lines(pst) == [dict(pop_st, round=1)]
    want, want_st = wm.model_rounds(popped, 5, **rule)
    assert [s["cut"] for s in want_st] == [1, 0] and want_st[1]["unitigs"] == 2
    assert _stats_lines(wst) == [dict(st, round=i + 1) for i, st in enumerate(want_st)]
    assert r.stdout.index("Graph cleaning round 1") < r.stdout.index("Bubble popping round 1") < r.stdout.index(
        "Weak-link removal round 1")
    got_units, got_edges, _ = _parse(gfa.read_text(), k)
    assert sorted(u[1] for u in got_units) == [100, 100] and not got_edges
    assert um.normalised(got_units) == um.normalised(cm.cdbg(want)[0])


def test_cli_cut_usage_errors(tmp_path):
    path = _fasta(tmp_path)
    out, gfa, f = tmp_path / "out.txt", tmp_path / "out.gfa", tmp_path / "cut.txt"
    base = [CLI, path, "21", "-s", "100000", "-o", str(out)]

    def run(*extra):
        return subprocess.run(base + list(extra), capture_output=True, text=True, cwd=tmp_path)

    requires = run("--gfa-min", "2").returncode  # the class of "A requires B"
    for extra in (["--cut-ratio", "100"], ["--cut-max-mean", "5"], ["--cut-rounds", "2"], ["--cut-min", "2"], ["--cut-max", "9"],
                  ["--cut-out", str(f)], ["--cut-stats", str(f)], ["--gfa", str(gfa), "--cut-rounds", "3"],
                  ["--clean-tips", "20", "--pop-bubbles", "21", "--cut-ratio", "100"]):
        r = run(*extra)
        assert r.returncode == requires != 0 and "require --cut-weak" in r.stderr, extra
    r = run("--cut-weak", "21", "--cut-min", "5", "--cut-max", "4")
    assert r.returncode != 0 and "minimum above its maximum" in r.stderr
    for opt in ("--cut-weak", "--cut-ratio", "--cut-max-mean", "--cut-rounds", "--cut-min", "--cut-max"):
        r = run("--cut-weak", "21", opt, "x")
        assert r.returncode != 0 and "Could not convert" in r.stderr, opt
    r = run("--cut-weak", "21", "--cut-rounds", "0")
    assert r.returncode != 0 and "--cut-rounds" in r.stderr
    r = run("--cut-weak", "21", "--cut-ratio", "1001")
    assert r.returncode != 0 and "--cut-ratio" in r.stderr and "0 to 1000" in r.stderr
    r = run("--cut-weak", "21", "--op", "union-sum", "--with", path)
    assert r.returncode != 0 and "excludes --op" in r.stderr
    assert not out.exists() and not gfa.exists() and not f.exists()  # nothing was counted or written
    text = subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout
    for opt in ("--cut-weak", "--cut-ratio", "--cut-max-mean", "--cut-rounds", "--cut-min,--cut-max", "--cut-out", "--cut-stats"):
        assert opt in text, opt
