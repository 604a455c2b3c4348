"""CPU: the unitig model (unitig_model.py) on hand-made tables -- the model is what the GPU tests
compare with, so its own answers are checked here on graphs small enough to read."""
import random

import numpy as np

import graph_model as g
import unitig_model as um
from kaarme_amd import UNITIG_CIRCULAR, unitig_strings


def table_of(reads, k):
    """{canonical k-mer: occurrences} of the reads"""
    t = {}
    for r in reads:
        for i in range(len(r) - k + 1):
            c = g.canon(r[i:i + k])
            t[c] = t.get(c, 0) + 1
    return t


def packed(units, k):
    """the model's unitigs as kc_unitigs would hand them over -- records (n, 4) and one bases array,
    here in reverse order with a gap between them -- read back with the package's unitig_strings"""
    records, parts, off = [], [], 0
    for s, n, total, circ in reversed(units):
        parts.append("N" * 3 + s)
        records.append((off + 3, n, total, UNITIG_CIRCULAR if circ else 0))
        off += 3 + len(s)
    records = np.array(records, dtype=np.uint64).reshape(-1, 4)
    bases = np.frombuffer("".join(parts).encode(), dtype=np.uint8)
    strings = unitig_strings(records, bases, k)
    return [(s, int(n), int(t), bool(f & UNITIG_CIRCULAR)) for s, (_, n, t, f) in zip(strings, records.tolist())]


def model(table, k, lo=1, hi=0):
    """um.unitigs, its strings checked and read back through the package's record layout"""
    units = um.unitigs(table, lo, hi)
    um.check_strings(units, k)
    assert packed(units, k) == units[::-1]
    return units


def _rand(seed, n):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(n))


def test_path_with_a_fork():
    k = 11
    stem, a, b = _rand(1, 60), "A" + _rand(2, 30), "C" + _rand(3, 30)
    table = table_of([stem + a, stem + b], k)
    units = model(table, k)
    st = um.stats(units, k)
    assert st["unitigs"] == 3 and st["circular"] == 0 and st["nodes"] == len(table) > st["unitigs"]
    names = {um.normal(s, n, c): (n, total) for s, n, total, c in units}
    # the stem up to the fork, counted twice; the two branches once
    assert names[g.canon(stem)] == (60 - k + 1, 2 * (60 - k + 1))
    assert names[g.canon((stem + a)[-(31 + k - 1):])] == (31, 31)
    assert names[g.canon((stem + b)[-(31 + k - 1):])] == (31, 31)
    # from 2 on only the stem is left: one unitig
    assert um.normalised(model(table, k, 2)) == [(g.canon(stem), 50, 100, False)]


def test_two_node_circle():
    k = 31
    table = table_of(["CA" * 40], k)
    assert len(table) == 2
    (s, n, total, circ), = model(table, k)
    assert (n, total, circ) == (2, 50, True) and len(s) == k + 1 and s[2:] == s[:k - 1]
    assert um.normal(s, n, circ) == "AC"


def test_poly_a_is_one_node_without_a_link():
    k = 31
    table = table_of(["A" * 60], k)
    assert model(table, k) in ([("A" * k, 1, 30, False)], [("T" * k, 1, 30, False)])


def test_hairpin_read():
    """(the read of test_gpu_graph.test_self_edges_never_link: it runs on into its own reverse
    complement, so the k-mers of its second half are those of the first and the turn links to itself)"""
    k = 31
    hair = "ACGGTCAATGCCTGAAGTCCATGACCGTTAGACT"
    table = table_of([hair + g.rc(hair)], k)
    units = model(table, k)
    st = um.stats(units, k)
    assert st["nodes"] == len(table) and st["circular"] == 0
    assert sum(total for _, _, total, _ in units) == sum(table.values())
    # every k-mer of every unitig is a node, and each node is spelled once
    spelled = [g.canon(s[i:i + k]) for s, n, _, _ in units for i in range(n)]
    assert sorted(spelled) == sorted(table)


def test_even_k_palindrome_stands_alone():
    k = 6
    pal = "AACGTT"
    assert pal == g.rc(pal)
    table = table_of(["GGC" + pal + "CAG"], k)
    units = model(table, k)
    assert (pal, 1, 1, False) in um.normalised(units)  # a palindrome has no link
    assert um.stats(units, k)["unitigs"] >= 3


def test_normal_names_both_strands_and_every_rotation():
    assert um.normal("ACGTT", 2, False) == um.normal(g.rc("ACGTT"), 2, False)
    k = 5
    circle = "ACGGTCATTG"
    names = set()
    for strand in (circle, g.rc(circle)):
        for i in range(len(circle)):
            rot = strand[i:] + strand[:i]
            names.add(um.normal(rot + rot[:k - 1], len(circle), True))
    assert len(names) == 1
