"""GPU: the drop-in CLI's --paths FILE --paths-out FILE [--paths-stats FILE] beside --gfa -- the records
of FILE threaded through the compacted graph, as GAF -- against KmerCounter.read_paths + gaf_lines on
the same input, against the GFA the same run writes, and against the model path_model.py."""
import re
import subprocess

import numpy as np
import pytest

from conftest import CLI
import cdbg_model as cm
import clean_cases as cc
import graph_model as m
import kaarme_amd as ka
import path_model as pm
import unitig_model as um
from test_gpu_cdbg_cli import _parse
from test_gpu_graph_cli import _fasta
from test_gpu_paths import fasta_seqs
from test_gpu_unitig import units_of
from test_gpu_unitig_cli import _with_circles

pytestmark = pytest.mark.gpu
K = 21
VISIT = re.compile(r"([<>])(\d+)")
STAT_NAMES = ("seqs", "windows", "located", "runs", "chains", "threaded")


def _reads_to_map(path):
    """(names, sequences): some of the counted reads as they are, in lower case, reversed, with an
    error and with an N, the 60-node circle 2.5 times round on both strands, a short and a foreign one"""
    seqs = fasta_seqs(open(path, "rb").read())
    circle = next(s for s in seqs if len(s) == 180)
    laps = (circle * 2)[7:7 + 150 + K - 1]
    rng = np.random.default_rng(12)
    bad = seqs[3][:40] + "ACGT"[("ACGT".index(seqs[3][40]) + 2) % 4] + seqs[3][41:]
    out = seqs[:12] + [seqs[12].lower(), m.rc(seqs[13]), bad, seqs[14][:30] + "N" + seqs[14][31:], laps, m.rc(laps),
                       "ACGTAC", "".join("ACGT"[i] for i in rng.integers(0, 4, 80)), "CA" * 30]
    return [f"q{i}" for i in range(len(out))], out


def _gaf(text, names, seqs, units, k):
    """the GAF lines checked against the segments `units` ([(string, n_nodes, count_sum, circular)]) and
    the queries, as comparable tuples: (name, qstart, qend, [(normal of the segment, strand in its
    normal form)], plen, pstart) -- a circle's strand, laps begun, plen and pstart depend on where it
    was cut: None"""
    out = []
    assert text == "" or text.endswith("\n")
    for line in text.splitlines():
        f = line.split("\t")
        assert len(f) == 13 and f[4] == "+" and f[11] == "255", line
        name, qlen, qs, qe, plen, ps, pe, matches, aln = f[0], int(f[1]), int(f[2]), int(f[3]), *map(int, f[6:11])
        i = names.index(name)
        visits = [(v.group(1) == "<", int(v.group(2))) for v in VISIT.finditer(f[5])]
        assert "".join(("<" if r else ">") + str(u) for r, u in visits) == f[5] and visits
        assert qlen == len(seqs[i]) and qe - qs == matches == aln == pe - ps and f[12] == f"cg:Z:{aln}="
        # the path spells the query interval when walked through the segments
        walk = ""
        for j, (rev, u) in enumerate(visits):
            s = cm.orient(units[u][0], rev)
            assert j == 0 or walk[len(walk) - (k - 1):] == s[:k - 1], line
            walk += s if j == 0 else s[k - 1:]
        assert plen == len(walk) and walk[ps:pe] == seqs[i][qs:qe].upper(), line
        norm = []
        for rev, u in visits:
            s, n, _, circ = units[u]
            nm = um.normal(s, n, circ)
            if circ:  # the laps begun depend on where the circle was cut too: one entry
                assert all(v == (rev, u) for v in visits)
                norm = [(nm, None)]
            else:
                norm.append((nm, int(rev) ^ (0 if s == m.rc(s) else int(s != nm))))
        on_circle = units[visits[0][1]][3]
        out.append((name, qs, qe, norm, None if on_circle else plen, None if on_circle else ps))
    return out


def _cli(tmp_path, path, reads_file, *extra):
    out, gfa, gaf, ps = (tmp_path / n for n in ("out.txt", "out.gfa", "out.gaf", "paths_stats.txt"))
    r = subprocess.run([CLI, path, str(K), "-s", "100000", "-a", "1", "-o", str(out), "--gfa", str(gfa), "--paths", str(reads_file),
                        "--paths-out", str(gaf), "--paths-stats", str(ps), *extra], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    table = {line.split()[0]: int(line.split()[1]) for line in out.read_text().splitlines()}
    stats = dict((l.split()[0], int(l.split()[1])) for l in ps.read_text().splitlines())
    return r, table, gfa.read_text(), gaf.read_text(), stats


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_cli_paths(fmt, tmp_path):
    path = _with_circles(tmp_path)
    names, seqs = _reads_to_map(path)
    reads_file = tmp_path / f"map.{fmt}"
    if fmt == "fastq":
        reads_file.write_text("".join(f"@{n} x\n{s}\n+\n{'I' * len(s)}\n" for n, s in zip(names, seqs)))
    else:
        reads_file.write_text("".join(f">{n} x\n{s[:50]}\n" + (f"{s[50:]}\n" if len(s) > 50 else "")
                                      for n, s in zip(names, seqs)))
    r, table, gfa_text, gaf_text, stats = _cli(tmp_path, path, reads_file)
    # the GFA beside the paths is a right answer for the table
    units, edges, cst = cm.cdbg(table)
    got_units, got_edges, _ = _parse(gfa_text, K)
    assert um.normalised(got_units) == um.normalised(units)
    assert cm.normalised_edges(got_units, got_edges) == cm.normalised_edges(units, edges)
    got = _gaf(gaf_text, names, seqs, got_units, K)
    # the Python call on the same input, written by gaf_lines
    kc, _ = ka.count_file(path, K, mode=2, min_abundance=1, table_slots=1 << 17)
    with kc:
        records, bases, _, _, runs, per, st = kc.read_paths(seqs)
        lines = ka.gaf_lines(names, seqs, records, runs, K)
        want = _gaf("".join(l + "\n" for l in lines), names, seqs, units_of(records, bases, K), K)
    assert got == want and len(got) == st["chains"] > len(seqs) - 4
    assert stats == st and list(stats) == list(STAT_NAMES)
    # ... and the model's
    text, off = pm.pack(seqs)
    assert pm.paths(table, text, off, K, graph=(units, edges, cst))[5] == st
    assert [g[0] for g in got if g[0] in ("q16", "q17")] == ["q16", "q17"]  # each lap-and-a-half is one line
    laps = [l.split("\t")[5] for l in gaf_text.splitlines() if l.split("\t")[0] in ("q16", "q17")]
    assert all(len(VISIT.findall(p)) in (3, 4) for p in laps) and laps[0][0] != laps[1][0]
    assert (f"Read paths: {st['seqs']} sequences, {st['windows']} k-mers, {st['located']} located, {st['runs']} runs, "
            f"{st['chains']} chains, {st['threaded']} threaded whole") in r.stdout.splitlines()


def test_cli_paths_follow_the_cleaned_table(tmp_path):
    path = _fasta(tmp_path)
    tip, branch = cc.chain_with_branch(K, t=3)  # a genome of 40 + 50 nodes and a tip of 3 off node 39
    with open(path, "ab") as f:
        f.write(cc.fasta(tip))
    seqs = fasta_seqs(open(path, "rb").read())[:40] + tip + [tip[0][30:40 + K - 1] + branch[K - 1:]]
    reads_file = tmp_path / "map.txt"
    reads_file.write_text("".join(s + "\n" for s in seqs))  # one per line: the names are the line numbers
    names = [str(i + 1) for i in range(len(seqs))]
    clean_out = tmp_path / "clean.txt"
    _, table, _, gaf_raw, raw = _cli(tmp_path, path, reads_file)
    _, _, gfa_text, gaf_text, stats = _cli(tmp_path, path, reads_file, "--clean-tips", str(K - 1), "--clean-out", str(clean_out))
    cleaned = {line.split()[0]: int(line.split()[1]) for line in clean_out.read_text().splitlines()}
    assert 0 < len(cleaned) < len(table)
    got_units, _, _ = _parse(gfa_text, K)
    units, edges, cst = cm.cdbg(cleaned)
    assert um.normalised(got_units) == um.normalised(units)
    text, off = pm.pack(seqs)
    _, _, _, runs, per, st = pm.paths(cleaned, text, off, K, graph=(units, edges, cst))
    # without its tip the genome is one unitig: its read is one run where it was two, the tip's k-mers are gone
    assert stats == st and stats["located"] <= raw["located"] - 3 - 3 and gaf_text != gaf_raw
    assert per[40] == {"first_run": per[40]["first_run"], "windows": 90, "located": 90, "runs": 1, "chains": 1, "longest_chain": 90}
    assert per[41]["located"] == 0 and per[42]["chains"] == 1 and per[42]["located"] == per[42]["windows"] - 3
    # the model's runs through gaf_lines
    records = np.array([[0, u[1], u[2], int(u[3])] for u in units], dtype=np.uint64).reshape(-1, 4)
    arr = np.zeros(len(runs), dtype=ka.RUN_DTYPE)
    for j, r_ in enumerate(runs):
        arr[j] = (r_["text_pos"], r_["seq"], r_["windows"], r_["unitig"], r_["pos"], r_["rev"] | r_["joined"] << 1, 0)
    want = _gaf("".join(l + "\n" for l in ka.gaf_lines(names, seqs, records, arr, K)), names, seqs, units, K)
    assert _gaf(gaf_text, names, seqs, got_units, K) == want


def test_cli_paths_usage_errors(tmp_path):
    path = _fasta(tmp_path)
    out, gfa, gaf, ps = (tmp_path / n for n in ("out.txt", "out.gfa", "out.gaf", "ps.txt"))
    base = [CLI, path, str(K), "-s", "100000", "-o", str(out)]

    def run(*extra):
        return subprocess.run(base + list(extra), capture_output=True, text=True, cwd=tmp_path)

    requires = run("--gfa-min", "2").returncode  # the class of "A requires B"
    for extra, msg in ((["--paths", path, "--paths-out", str(gaf)], "--paths requires --gfa"),
                       (["--gfa", str(gfa), "--paths", path], "--paths requires --paths-out"),
                       (["--gfa", str(gfa), "--paths-out", str(gaf)], "--paths-out requires --paths"),
                       (["--gfa", str(gfa), "--paths-stats", str(ps)], "--paths-stats requires --paths")):
        r = run(*extra)
        assert r.returncode == requires != 0 and msg in r.stderr, extra
    r = run("--gfa", str(gfa), "--paths", str(tmp_path / "none.fa"), "--paths-out", str(gaf))
    assert r.returncode != 0 and "--paths: File does not exist" in r.stderr
    assert not out.exists() and not gfa.exists() and not gaf.exists() and not ps.exists()  # nothing was counted or written
    assert "--paths-out" in subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout
