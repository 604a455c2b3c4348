"""GPU: the drop-in CLI's bubble popping -- --pop-bubbles N, --pop-max-diff D, --pop-max-mean M,
--pop-rounds R, --pop-min/--pop-max N, --pop-out FILE, --pop-stats FILE -- against the pure-Python
model bubble_model.py on the counts the same run writes with -a 1: --gfa then reads the popped table,
-o still the counted one, and with --clean-* the cleaning runs first."""
import subprocess

import pytest

from conftest import CLI
import bubble_cases as bc
import bubble_model as bm
import cdbg_model as cm
import clean_cases as cc
import clean_model as clm
import unitig_model as um
from test_gpu_cdbg_cli import _parse
from test_gpu_clean_cli import _stats_lines, _table
from test_gpu_graph_cli import _fasta

pytestmark = pytest.mark.gpu


def _run(args, cwd):
    r = subprocess.run(args, capture_output=True, text=True, cwd=cwd)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_pop_bubble_to_one_segment(tmp_path):
    k = 31
    (g0, alt), _ = cc.bubble(k)
    path = tmp_path / "bubble.fasta"
    path.write_bytes(cc.fasta([g0] * 3 + [alt]))
    out, gfa, pout, pst = tmp_path / "out.txt", tmp_path / "out.gfa", tmp_path / "pop.txt", tmp_path / "pop.stats"
    base = [CLI, str(path), str(k), "-s", "100000", "-a", "1"]
    _run(base + ["-o", str(out), "--gfa", str(gfa)], tmp_path)
    assert len(_parse(gfa.read_text(), k)[0]) == 4  # without the option the bubble is there
    r = _run(base + ["-o", str(out), "--gfa", str(gfa), "--pop-bubbles", str(k), "--pop-out", str(pout), "--pop-stats", str(pst)],
             tmp_path)
    table = _table(out)
    want, want_st = bm.pop(table, max_nodes=k)
    assert want_st["popped"] == 1 and len(want) == 100
    assert _stats_lines(pst) == [dict(want_st, round=1)] and r.stdout.count("Bubble popping round ") == 1
    assert _table(pout) == want and sorted(pout.read_text().splitlines()) == sorted(f"{c} {t}" for c, t in want.items())
    got_units, got_edges, closing = _parse(gfa.read_text(), k)
    assert len(got_units) == 1 and got_units[0][1] == 100 and not got_edges and not closing
    assert um.normalised(got_units) == um.normalised(cm.cdbg(want)[0])


def test_cli_pop_rounds_and_clean_first(tmp_path):
    """the variants of bubble_cases, and a tip off the genome's arm of the first site: that arm is two
    unitigs until --clean-tips has removed the tip, so the site's bubble is popped only after cleaning"""
    k = 21
    seqs, alts = bc.variants(k)
    import numpy as np
    tip = cc.branch(np.random.default_rng(4), seqs[0], 3 * k - 5, 4, k)
    path = tmp_path / "variants.fasta"
    path.write_bytes(cc.fasta(seqs + [tip]))
    out, gfa, pst, cst = tmp_path / "out.txt", tmp_path / "out.gfa", tmp_path / "pop.stats", tmp_path / "clean.stats"
    base = [CLI, str(path), str(k), "-s", "100000", "-a", "1", "-o", str(out)]
    pop = ["--pop-bubbles", str(k), "--pop-max-diff", "1", "--pop-rounds", "5", "--pop-stats", str(pst)]
    # popping alone: the first site's variant is a branch without a parallel one
    _run(base + pop + ["--gfa", str(gfa)], tmp_path)
    table = _table(out)
    rule = dict(max_nodes=k, max_diff=1)
    want, want_st = bm.model_rounds(table, 5, **rule)
    assert [s["popped"] for s in want_st] == [4, 0] and want_st[0]["branches"] > want_st[0]["parallel"]
    assert _stats_lines(pst) == [dict(st, round=i + 1) for i, st in enumerate(want_st)]
    units, edges, _ = cm.cdbg(want)
    got_units, got_edges, _ = _parse(gfa.read_text(), k)
    assert um.normalised(got_units) == um.normalised(units) and len(units) > 1
    assert cm.normalised_edges(got_units, got_edges) == cm.normalised_edges(units, edges)
    # cleaning first, then popping on the table it left: one chain
    r = _run(base + ["--clean-tips", str(k - 1), "--clean-stats", str(cst)] + pop + ["--gfa", str(gfa)], tmp_path)
    cleaned, clean_st = clm.clean(table, 1, 0, tip_max_nodes=k - 1)
    assert clean_st["tips"] == 1 and _stats_lines(cst) == [dict(clean_st, round=1)]
    want, want_st = bm.model_rounds(cleaned, 5, **rule)
    assert [s["popped"] for s in want_st] == [5, 0]
    assert _stats_lines(pst) == [dict(st, round=i + 1) for i, st in enumerate(want_st)]
    assert r.stdout.index("Graph cleaning round 1") < r.stdout.index("Bubble popping round 1")
    got_units, got_edges, _ = _parse(gfa.read_text(), k)
    assert len(got_units) == 1 and not got_edges and um.normalised(got_units) == um.normalised(cm.cdbg(want)[0])
    # the range and the guard: from T(c) >= 2 on the genome is one chain; no arm has a mean of 1 or less but the variants'
    _run(base + ["--digest-only", "--pop-bubbles", str(k), "--pop-min", "2", "--pop-stats", str(pst)], tmp_path)
    assert _stats_lines(pst) == [dict(bm.pop(table, 2, 0, max_nodes=k)[1], round=1)]
    _run(base + ["--digest-only", "--pop-bubbles", str(k), "--pop-max-mean", "1", "--pop-max", "9", "--pop-stats", str(pst)], tmp_path)
    st = bm.pop(table, 1, 9, max_nodes=k, max_mean=1)[1]
    assert st["popped"] == 3 and _stats_lines(pst) == [dict(st, round=1)]


def test_cli_pop_usage_errors(tmp_path):
    path = _fasta(tmp_path)
    out, gfa, f = tmp_path / "out.txt", tmp_path / "out.gfa", tmp_path / "pop.txt"
    base = [CLI, path, "21", "-s", "100000", "-o", str(out)]

    def run(*extra):
        return subprocess.run(base + list(extra), capture_output=True, text=True, cwd=tmp_path)

    requires = run("--gfa-min", "2").returncode  # the class of "A requires B"
    for extra in (["--pop-max-diff", "1"], ["--pop-max-mean", "5"], ["--pop-rounds", "2"], ["--pop-min", "2"], ["--pop-max", "9"],
                  ["--pop-out", str(f)], ["--pop-stats", str(f)], ["--gfa", str(gfa), "--pop-rounds", "3"],
                  ["--clean-tips", "20", "--pop-max-diff", "1"]):
        r = run(*extra)
        assert r.returncode == requires != 0 and "require --pop-bubbles" in r.stderr, extra
    r = run("--pop-bubbles", "21", "--pop-min", "5", "--pop-max", "4")
    assert r.returncode != 0 and "minimum above its maximum" in r.stderr
    for opt in ("--pop-bubbles", "--pop-max-diff", "--pop-max-mean", "--pop-rounds", "--pop-min", "--pop-max"):
        r = run("--pop-bubbles", "21", opt, "x")
        assert r.returncode != 0 and "Could not convert" in r.stderr, opt
    r = run("--pop-bubbles", "21", "--pop-rounds", "0")
    assert r.returncode != 0 and "--pop-rounds" in r.stderr
    r = run("--pop-bubbles", "21", "--op", "union-sum", "--with", path)
    assert r.returncode != 0 and "excludes --op" in r.stderr
    assert not out.exists() and not gfa.exists() and not f.exists()  # nothing was counted or written
    assert "--pop-bubbles" in subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout
