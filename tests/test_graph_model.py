"""CPU: the de Bruijn graph model (graph_model.py) on hand-made graphs whose flags are written out
here, and the properties the contract states: links are mutual and lead back, side_degree sums to
2 * nodes, link_ends is even."""
import itertools
import random

import pytest

import graph_model as m


def table(seqs, k):
    t = {}
    for s in seqs:
        for i in range(len(s) - k + 1):
            c = m.canon(s[i:i + k])
            t[c] = t.get(c, 0) + 1
    return t


def stats(nodes, edge_ends, link_ends, isolated, palindromes, side_degree):
    return {"nodes": nodes, "edge_ends": edge_ends, "link_ends": link_ends, "isolated": isolated,
            "palindromes": palindromes, "side_degree": side_degree, "open_unitigs": nodes - link_ends // 2}


def test_simple_path():
    """ACCG -> CCGA -> CGAT -> GATT; the last two are stored as ATCG and AATC, read backwards: one
    unitig, open at both ends"""
    t = table(["ACCGATT"], 4)
    assert t == {"ACCG": 1, "CCGA": 1, "ATCG": 1, "AATC": 1}
    flags, st = m.graph(t)
    assert flags == {"ACCG": 0x8101,   # R: A (CCGA), linked; no L
                     "CCGA": 0x8318,   # R: T (CGAT = rc ATCG), L: A (ACCG), both linked
                     "ATCG": 0x8314,   # R: G (TCGG = rc CCGA), L: A (AATC), both linked
                     "AATC": 0x8104}   # R: G (ATCG), linked; no L
    assert st == stats(4, 6, 6, 0, 0, [2, 6, 0, 0, 0]) and st["open_unitigs"] == 1


def test_fork():
    """CCGA is followed by T and by G: its side R has degree 2, so neither successor links back"""
    t = table(["ACCGATT", "CCGAG"], 4)
    flags, st = m.graph(t)
    assert flags == {"ACCG": 0x8101, "CCGA": 0x821C, "ATCG": 0x8214, "AATC": 0x8104, "CGAG": 0x8020}
    assert st == stats(5, 8, 4, 0, 0, [3, 6, 1, 0, 0]) and st["open_unitigs"] == 3


def test_tip_and_the_range_that_removes_it():
    """an error k-mer CCGC seen once hangs off ACCG: a fork at min_count 1, gone at min_count 2 --
    the nodes outside the range are no neighbours either"""
    t = table(["ACCGATT", "ACCGATT", "CCGC"], 4)
    flags, st = m.graph(t)
    assert flags == {"ACCG": 0x8003, "CCGA": 0x8118, "ATCG": 0x8314, "AATC": 0x8104, "CCGC": 0x8010}
    assert st == stats(5, 8, 4, 0, 0, [3, 6, 1, 0, 0])
    flags, st = m.graph(t, min_count=2)
    assert flags == {"ACCG": 0x8101, "CCGA": 0x8318, "ATCG": 0x8314, "AATC": 0x8104}
    assert st == stats(4, 6, 6, 0, 0, [2, 6, 0, 0, 0])
    assert m.graph(t, min_count=0) == m.graph(t, min_count=1)
    assert m.graph(t, max_count=1)[0] == {"CCGC": 0x8000} and m.graph(t, max_count=1)[1]["isolated"] == 1
    assert m.graph(t, min_count=2, max_count=2) == m.graph(t, min_count=2)


def test_poly_a_self_loop():
    """AAAA follows and precedes itself: both sides have degree 1 and neither links"""
    flags, st = m.graph(table(["AAAAAAA"], 4))
    assert flags == {"AAAA": 0x8011}
    assert st == stats(1, 2, 0, 0, 0, [0, 2, 0, 0, 0])


def test_hairpin():
    """GACGT is followed by ACGTC, its own reverse complement: one node whose side L leads to itself"""
    t = table(["GACGTC"], 5)
    assert t == {"ACGTC": 2}
    flags, st = m.graph(t)
    assert flags == {"ACGTC": 0x8040}
    assert st == stats(1, 1, 0, 0, 0, [1, 1, 0, 0, 0])


def test_even_k_palindrome():
    """CACG -> ACGT -> CGTG (= rc CACG) -> GTGA: ACGT is its own reverse complement, so the edges to
    it are there and no link touches it; CACG and GTGA link through their L sides"""
    t = table(["CACGTGA"], 4)
    assert t == {"CACG": 2, "ACGT": 1, "GTGA": 1}
    flags, st = m.graph(t)
    assert flags == {"ACGT": 0x8024, "CACG": 0x8288, "GTGA": 0x8220}
    assert st == stats(3, 5, 2, 0, 1, [1, 5, 0, 0, 0])
    assert m.link_partner(set(t), "CACG", "L") == ("GTGA", "L")


def test_neighbors_swap_and_complement_on_the_other_strand():
    t = table(["ACCGATT", "CCGAG"], 4)
    assert m.neighbors(t, "CCGA") == [0, 0, 1, 1, 1, 0, 0, 0]
    assert m.neighbors(t, "TCGG") == [0, 0, 0, 1, 1, 1, 0, 0]
    for x in ("CCGA", "ATCG", "GGGG"):
        fwd, rev = m.neighbors(t, x), m.neighbors(t, m.rc(x))
        assert [rev[4 + 3 - y] for y in range(4)] == fwd[:4] and [rev[3 - y] for y in range(4)] == fwd[4:]


def test_node_line():
    assert m.node_line("CCGA", 2, 0x821C) == "CCGA 2 ..GT A... L-"
    assert m.node_line("ACGT", 7, 0x8300) == "ACGT 7 .... .... LR"


@pytest.mark.parametrize("k", [2, 3, 4, 5, 6, 7])
def test_links_are_mutual_on_random_node_sets(k):
    allk = sorted({m.canon("".join(p)) for p in itertools.product(m.BASES, repeat=k)})
    links = 0
    for trial in range(100):
        rng = random.Random(trial * 10 + k)
        nodes = set(rng.sample(allk, rng.randint(1, min(len(allk), 60))))
        flags, st = m.graph(dict.fromkeys(nodes, 1))
        for c in nodes:
            for s, bit in (("R", m.LINK_R), ("L", m.LINK_L)):
                if flags[c] & bit:
                    links += 1
                    d, t = m.link_partner(nodes, c, s)
                    assert flags[d] & (m.LINK_R if t == "R" else m.LINK_L), (c, s, d, t)
                    assert m.link_partner(nodes, d, t) == (c, s)
        assert sum(st["side_degree"]) == 2 * st["nodes"] == 2 * len(nodes)
        assert st["link_ends"] % 2 == 0 and st["link_ends"] == sum(bin(f & 0x300).count("1") for f in flags.values())
        assert st["edge_ends"] == sum(i * n for i, n in enumerate(st["side_degree"]))
        assert all(f & 0x7C00 == 0 and f & m.NODE for f in flags.values())
    assert links > 0
