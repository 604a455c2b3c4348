"""The read-path model (path_model.py) on hand-made cases with the answers written out (CPU).  The
model asserts the header's properties on every input it is given; these cases pin its answers."""
import numpy as np

import clean_cases as cc
import graph_model as m
import path_model as pm

K = 15


def run(seqs_counted, reads, k=K, min_count=1, max_count=0, text=None, offsets=None):
    table = pm.count(seqs_counted, k)
    if text is None:
        text, offsets = pm.pack(reads)
    return pm.paths(table, text, offsets, k, min_count, max_count)


def shape(runs):
    return [(r["seq"], r["text_pos"], r["windows"], r["joined"]) for r in runs]


def test_chain_with_branch():
    seqs, b = cc.chain_with_branch(K)
    g = seqs[0]
    cross = g[35:40 + K - 1] + b[K - 1:]  # nodes 35 .. 39 of the genome, then the branch
    units, edges, _, runs, per, st = run(seqs, [g, b, cross])
    assert sorted(u[1] for u in units) == [3, 40, 50]
    o = [0, len(g) + 1, len(g) + len(b) + 2]
    assert shape(runs) == [(0, 0, 40, 0), (0, 40, 50, 1), (1, o[1], 3, 0), (2, o[2], 5, 0), (2, o[2] + 5, 3, 1)]
    assert runs[0]["pos"] == 0 and runs[1]["pos"] == 0 and runs[3]["pos"] == 35 and runs[4]["pos"] == 0
    assert runs[2]["unitig"] == runs[4]["unitig"] and runs[0]["unitig"] == runs[3]["unitig"]
    assert per[0] == {"first_run": 0, "windows": 90, "located": 90, "runs": 2, "chains": 1, "longest_chain": 90}
    assert per[2] == {"first_run": 3, "windows": 8, "located": 8, "runs": 2, "chains": 1, "longest_chain": 8}
    assert st == {"seqs": 3, "windows": 101, "located": 101, "runs": 5, "chains": 3, "threaded": 3}


def test_bubble_and_tip():
    seqs, _ = cc.bubble(K)
    _, _, _, runs, per, st = run(seqs, [seqs[0], m.rc(seqs[0])])
    n = len(seqs[0]) + 1
    assert shape(runs) == [(0, 0, 50, 0), (0, 50, K, 1), (0, 50 + K, 50 - K, 1),
                           (1, n, 50 - K, 0), (1, n + 50 - K, K, 1), (1, n + 50, 50, 1)]
    # the reverse read walks the same unitigs backwards on the other strand
    assert [r["unitig"] for r in runs[3:]] == [r["unitig"] for r in runs[2::-1]]
    assert [r["rev"] for r in runs[3:]] == [1 - r["rev"] for r in runs[2::-1]]
    assert st["threaded"] == 2 and per[1]["longest_chain"] == 100
    seqs, stem = cc.two_tip_junction(K)
    _, _, _, runs, per, _ = run(seqs, [seqs[1]])
    assert shape(runs) == [(0, 0, 50, 0), (0, 50, 3, 1)] and per[0]["chains"] == 1


def test_hairpin():
    rng = np.random.default_rng(21)
    r = cc.rand(rng, 40)
    x = r + m.rc(r)  # windows p and 80 - K - p are each other's reverse complement
    nodes = 40 - (K - 1) // 2
    units, edges, _, runs, per, _ = run([x], [x])
    assert [u[1] for u in units] == [nodes]
    assert shape(runs) == [(0, 0, nodes, 0), (0, nodes, nodes, 1)]
    assert runs[0]["unitig"] == runs[1]["unitig"] == 0 and runs[0]["rev"] != runs[1]["rev"]
    assert runs[0]["pos"] == runs[1]["pos"] == 0
    assert (0, runs[0]["rev"], 0, runs[1]["rev"]) in edges
    assert per[0]["longest_chain"] == 2 * nodes == per[0]["windows"]


def test_homopolymer():
    units, edges, _, runs, per, st = run(["A" * 8], ["A" * 8, "T" * 7], k=5)
    assert units == [("AAAAA", 1, 4, False)] and sorted(edges) == [(0, 0, 0, 0), (0, 1, 0, 1)]
    # every window is a run of its own, joined to the one before through (U, +, U, +)
    assert shape(runs) == [(0, 0, 1, 0), (0, 1, 1, 1), (0, 2, 1, 1), (0, 3, 1, 1), (1, 9, 1, 0), (1, 10, 1, 1), (1, 11, 1, 1)]
    assert [r["rev"] for r in runs] == [0] * 4 + [1] * 3 and all(r["pos"] == 0 for r in runs)
    assert per[0] == {"first_run": 0, "windows": 4, "located": 4, "runs": 4, "chains": 1, "longest_chain": 4}
    assert st["threaded"] == 2


def test_circle_two_point_four_laps():
    rng = np.random.default_rng(3)
    c = cc.rand(rng, 5)
    circle = c * 8
    read = circle[2:2 + 12 + K - 1]  # 12 windows round a circle of 5 nodes
    units, edges, _, runs, per, st = run([circle], [read, m.rc(read)])
    assert [(u[1], u[3]) for u in units] == [(5, True)] and edges == []
    n = len(read) + 1
    assert shape(runs) == [(0, 0, 12, 0), (1, n, 12, 0)]
    assert runs[0]["rev"] != runs[1]["rev"] and all(r["pos"] < 5 for r in runs)
    assert per[0]["runs"] == per[1]["runs"] == 1 and st["threaded"] == 2


def test_palindromic_node():
    for k, s in ((4, "TTACGTCA"), (6, "GTAACGTTCA")):
        pal = s[2:2 + k]
        assert pal == m.rc(pal)
        units, edges, _, runs, per, _ = run([s], [s, m.rc(s)], k=k)
        assert sorted(u[1] for u in units) == [1, 2, 2]
        n = len(s) + 1
        assert shape(runs) == [(0, 0, 2, 0), (0, 2, 1, 1), (0, 3, 2, 1), (1, n, 2, 0), (1, n + 2, 1, 1), (1, n + 3, 2, 1)]
        # a palindromic unitig has one orientation
        assert runs[1]["rev"] == 0 and runs[4]["rev"] == 0 and runs[1]["unitig"] == runs[4]["unitig"]
        assert units[runs[1]["unitig"]][0] == pal
        assert per[0]["longest_chain"] == 5


def test_error_in_the_middle():
    rng = np.random.default_rng(8)
    g = cc.rand(rng, 200)
    read = g[10:70]
    bad = read[:30] + cc.BASES[(cc.BASES.index(read[30]) + 1) % 4] + read[31:]
    _, _, _, runs, per, st = run([g], [bad])
    assert shape(runs) == [(0, 0, 16, 0), (0, 31, 15, 0)]
    assert runs[0]["pos"] in (10, 200 - K - 10 - 15) and runs[0]["unitig"] == runs[1]["unitig"]
    assert per[0] == {"first_run": 0, "windows": 46, "located": 31, "runs": 2, "chains": 2, "longest_chain": 16}
    assert st["threaded"] == 0


def test_breaks_case_short_and_empty():
    rng = np.random.default_rng(9)
    g = cc.rand(rng, 100)
    withn = g[:40] + "N" + g[41:80]
    _, _, _, runs, per, st = run([g], [g.lower(), withn, g[:K - 1], "", g[50:50 + K]])
    assert shape(runs)[0] == (0, 0, 100 - K + 1, 0)
    # the windows that hold the N are no windows; the two sides are two chains of one unitig
    assert per[1] == {"first_run": 1, "windows": 80 - K + 1 - K, "located": 80 - K + 1 - K, "runs": 2, "chains": 2,
                      "longest_chain": 40 - K + 1}
    assert per[2] == {"first_run": 3, "windows": 0, "located": 0, "runs": 0, "chains": 0, "longest_chain": 0}
    assert per[3] == per[2]
    assert per[4] == {"first_run": 3, "windows": 1, "located": 1, "runs": 1, "chains": 1, "longest_chain": 1}
    assert st["seqs"] == 5 and st["threaded"] == 2 and st["runs"] == 4


def test_adjacent_sequences_share_no_window():
    rng = np.random.default_rng(10)
    g = cc.rand(rng, 60)
    _, _, _, runs, per, st = run([g], None, text=g, offsets=[0, 30, 60])
    assert shape(runs) == [(0, 0, 16, 0), (1, 30, 16, 0)]
    assert runs[1]["pos"] - runs[0]["pos"] in (30, -30)
    assert [p["windows"] for p in per] == [16, 16] and st["windows"] == 32 and st["threaded"] == 2


def test_range_and_empty_table():
    rng = np.random.default_rng(11)
    g = cc.rand(rng, 80)
    # the second half is counted twice: with min_count = 2 only its nodes are in the range
    units, _, _, runs, per, st = run([g, g[40:]], [g], min_count=2)
    assert [u[1] for u in units] == [40 - K + 1]
    assert shape(runs) == [(0, 40, 40 - K + 1, 0)] and per[0]["windows"] == 80 - K + 1
    _, _, _, runs, per, st = pm.paths({}, g + "\n", [0, 81], K)
    assert runs == [] and st == {"seqs": 1, "windows": 66, "located": 0, "runs": 0, "chains": 0, "threaded": 0}
