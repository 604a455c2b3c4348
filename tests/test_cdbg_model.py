"""CPU: the compacted-graph model (cdbg_model.py) on hand-made tables -- the model is what the GPU
tests compare with, so its own answers are checked here against edge lists written out by hand, and
the package's gfa_lines against the text they spell."""
import numpy as np

import cdbg_model as cm
import graph_model as g
import unitig_model as um
from kaarme_amd import EDGE_DTYPE, EDGE_FROM_REV, EDGE_TO_REV, UNITIG_CIRCULAR, gfa_lines
from test_unitig_model import table_of


def by_hand(edges):
    """[(string of U, from_rev, string of V, to_rev)] with the strings as the hand chose to read
    them, in normalised_edges' form"""
    def name(s, rev):
        nm = g.canon(s)
        return nm, rev ^ (0 if s == g.rc(s) else int(s != nm))
    return sorted(name(a, fr) + name(b, tr) for a, fr, b, tr in edges)


def model(table, k, lo=1, hi=0):
    units, edges, st = cm.cdbg(table, lo, hi)
    um.check_strings(units, k)
    assert st["edges"] == len(edges) and all(len(e) == 4 for e in edges)
    return units, edges, st


def packed(units, edges):
    """the model's graph as kc_unitig_graph hands it over: records (n, 4), one bases array, EDGE_DTYPE edges"""
    records, off = [], 0
    for s, n, total, circ in units:
        records.append((off, n, total, UNITIG_CIRCULAR if circ else 0))
        off += len(s)
    arr = np.zeros(len(edges), dtype=EDGE_DTYPE)
    for j, (u, fr, v, tr) in enumerate(edges):
        arr[j] = (u, v, (EDGE_FROM_REV if fr else 0) | (EDGE_TO_REV if tr else 0), 0)
    bases = np.frombuffer("".join(u[0] for u in units).encode(), dtype=np.uint8)
    return np.array(records, dtype=np.uint64).reshape(-1, 4), bases, arr


def test_y_fork():
    k = 5
    stem, a, b = "ACCACTGGGT", "AAGGA", "CTACG"
    table = table_of([stem + a, stem + b], k)
    units, edges, st = model(table, k)
    sa, sb = stem[-(k - 1):] + a, stem[-(k - 1):] + b
    assert sorted(um.normal(s, n, c) for s, n, _, c in units) == sorted(g.canon(x) for x in (stem, sa, sb))
    # the stem runs on into both branches, and each branch, read backwards, into the stem read backwards
    assert cm.normalised_edges(units, edges) == by_hand([(stem, 0, sa, 0), (stem, 0, sb, 0), (sa, 1, stem, 1),
                                                          (sb, 1, stem, 1)])
    assert (st["unitigs"], st["edges"], st["dead_ends"]) == (3, 4, 3)
    # from 2 on only the stem's first nodes are left: one unitig, no edge, two dead ends
    units, edges, st = model(table, k, 2)
    assert (st["unitigs"], st["edges"], st["dead_ends"]) == (1, 0, 2) and edges == []
    assert cm.edge_tuples(packed(units, edges)[2]) == edges


def test_hairpin_is_its_own_mirror():
    k = 5
    half = "ACGGTCA"
    table = table_of([half + g.rc(half)], k)
    units, edges, st = model(table, k)
    # ACGGT .. TCATG, whose successor CATGA is TCATG read backwards: the end of U+ runs on into U-
    u = "ACGGTCATG"
    assert um.normalised(units) == [(g.canon(u), 5, 10, False)]
    assert cm.normalised_edges(units, edges) == by_hand([(u, 0, u, 1)]) and len(edges) == 1
    assert (st["edges"], st["dead_ends"]) == (1, 1)


def test_homopolymer_has_both_loops():
    k = 4
    table = table_of(["AAAAAA"], k)
    units, edges, st = model(table, k)
    assert um.normalised(units) == [("AAAA", 1, 3, False)]
    assert cm.normalised_edges(units, edges) == by_hand([("AAAA", 0, "AAAA", 0), ("AAAA", 1, "AAAA", 1)])
    assert (st["edges"], st["dead_ends"]) == (2, 0)


def test_palindromic_node_reports_side_r_only():
    k = 4
    pal, a, c = "ACGT", "CGTA", "CGTC"
    table = table_of(["T" + pal + "C"], k)
    assert sorted(table) == sorted([pal, a, c]) and pal == g.rc(pal)
    units, edges, st = model(table, k)
    assert sorted(u[0] for u in um.normalised(units)) == sorted([pal, a, c])
    # ACGT is followed by CGTA and CGTC; read backwards it is itself, so what precedes it (TACG, GACG)
    # are the same two nodes and side L adds nothing.  Its bit is 0 on either end of an edge.
    assert cm.normalised_edges(units, edges) == by_hand([(pal, 0, a, 0), (pal, 0, c, 0), (a, 1, pal, 0), (c, 1, pal, 0)])
    assert cm.palindromic_left_ends(table) == 2
    assert g.graph(table)[1]["edge_ends"] == 6 and g.graph(table)[1]["link_ends"] == 0
    assert (st["unitigs"], st["edges"], st["dead_ends"]) == (3, 4, 2)
    records, bases, arr = packed(units, edges)
    assert cm.edge_tuples(arr) == edges
    lines = gfa_lines(records, bases, arr, k)
    assert lines[0] == "H\tVN:Z:1.0" and len(lines) == 1 + 3 + 4
    i = {u[0]: j for j, u in enumerate(units)}
    assert f"S\t{i[pal]}\t{pal}\tLN:i:4\tKC:i:1" in lines[1:4]
    assert sum(l.startswith(f"L\t{i[pal]}\t+\t") and l.endswith("\t3M") for l in lines[4:]) == 2
    assert sum(l.startswith("L\t") and f"\t{i[pal]}\t+\t3M" in l for l in lines[4:]) == 2


def test_circle_has_no_edges():
    k = 5
    circle = "GCGGAGGGCA"
    table = table_of([circle * 3], k)
    units, edges, st = model(table, k)
    assert [(u[1], u[3]) for u in units] == [(10, True)] and edges == []
    assert (st["circular"], st["edges"], st["dead_ends"]) == (1, 0, 0)
    records, bases, arr = packed(units, edges)
    s = units[0][0]
    assert gfa_lines(records, bases, arr, k) == ["H\tVN:Z:1.0", f"S\t0\t{s}\tLN:i:14\tKC:i:{units[0][2]}",
                                                 "L\t0\t+\t0\t+\t4M", "L\t0\t-\t0\t-\t4M"]


def test_gfa_lines_of_a_fork():
    k = 5
    units = [("ACCACTGGGT", 6, 12, False), ("GGGTAAGGA", 5, 5, False)]
    records, bases, arr = packed(units, [(0, 0, 1, 0), (1, 1, 0, 1)])
    assert gfa_lines(records, bases, arr, k) == [
        "H\tVN:Z:1.0", "S\t0\tACCACTGGGT\tLN:i:10\tKC:i:12", "S\t1\tGGGTAAGGA\tLN:i:9\tKC:i:5",
        "L\t0\t+\t1\t+\t4M", "L\t1\t-\t0\t-\t4M"]
