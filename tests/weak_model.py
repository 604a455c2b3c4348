"""Pure-Python model of weak-link removal (include/kc_api.h kc_cut_weak*) over a {k-mer string: T(c)}
dict of canonical k-mers, built on cdbg_model.cdbg: the unitigs of the range's graph and the edges
between them.

  interior    U is open and not palindromic, and both ends have degree >= 1 (clean_model.end_degrees:
              the edges with from == U, self edges included)
  neighbours  N(U): one entry V for every edge (U, from_rev, V, to_rev) with V != U -- a multiset, at
              most eight entries; edges back into U give none
  local       local_sum, local_n: count_sum and n summed over N(U)
  weak        N(U) is not empty, and ratio_permille == 0 or
              count_sum(U) * local_n * 1000 < ratio_permille * local_sum * n(U)   (Python integers: exact)
  cut         max_nodes != 0, n(U) <= max_nodes, the guard passes, U is interior and weak
Every verdict is taken on the one graph; the nodes of every other unitig are kept with their raw
counts.  The model asserts on every input: the node balance; that nothing circular, palindromic, a
tip or isolated is cut; with ratio_permille in 1..1000, that every cut unitig has a neighbour whose
mean is strictly higher and that no unitig with the highest mean of the graph is cut."""
from fractions import Fraction

import cdbg_model as cm
import clean_model as clm
import graph_model as m

FIELDS = ("unitigs", "nodes", "interior", "weak", "cut", "cut_nodes", "out_keys", "out_sum")


def neighbours(units, edges):
    """[N(U) as a list of unitig indices, one per edge that leaves U for another unitig] per unitig"""
    out = [[] for _ in units]
    for u, _, v, _ in edges:
        if v != u:
            out[u].append(v)
    return out


def interior(units, edges):
    """the set of the interior unitigs' indices"""
    deg = clm.end_degrees(units, edges)
    return {u for u, (s, n, _, circ) in enumerate(units)
            if not circ and s != m.rc(s) and deg[u][0] >= 1 and deg[u][1] >= 1}


def local(units, entries):
    """(local_sum, local_n) over the entries of one N(U)"""
    return sum(units[v][2] for v in entries), sum(units[v][1] for v in entries)


def is_weak(unit, local_sum, local_n, entries, ratio_permille):
    return bool(entries) and (ratio_permille == 0 or unit[2] * local_n * 1000 < ratio_permille * local_sum * unit[1])


def cut(table, min_count=1, max_count=0, max_nodes=0, ratio_permille=0, max_mean=0, raw=None, graph=None):
    """(kept {k-mer: raw count}, the kc_weak_stats dict).  table holds T(c); raw (default: none
    differs) the raw counts of the k-mers whose raw count is not their T(c); graph: cdbg_model.cdbg
    of the same table and range, when it is at hand."""
    assert 0 <= ratio_permille <= 1000, "KC_ERR_ARG"
    assert not (max_nodes and not ratio_permille and not max_mean), "KC_ERR_ARG"
    units, edges, cst = graph or cm.cdbg(table, min_count, max_count)
    raw = raw or {}
    st = dict.fromkeys(FIELDS, 0)
    st["unitigs"], st["nodes"] = cst["unitigs"], cst["nodes"]
    inside, nb = interior(units, edges), neighbours(units, edges)
    deg = clm.end_degrees(units, edges)
    st["interior"] = len(inside)
    gone = set()
    for u in sorted(inside):
        s, n, total, _ = units[u]
        assert len(nb[u]) <= 8, "N(U) has at most eight entries"
        assert all(not units[v][3] for v in nb[u]), "neighbours are open unitigs"
        local_sum, local_n = local(units, nb[u])
        if not is_weak(units[u], local_sum, local_n, nb[u], ratio_permille):
            continue
        st["weak"] += 1
        if max_nodes and n <= max_nodes and (max_mean == 0 or total <= max_mean * n):
            gone.add(u)
    top = max((Fraction(un[2], un[1]) for un in units), default=0)
    for u in gone:
        s, n, total, circ = units[u]
        assert not circ and s != m.rc(s) and clm.category(units[u], deg[u]) is None
        if ratio_permille:
            assert any(units[v][2] * n > total * units[v][1] for v in nb[u]), "a neighbour's mean is strictly higher"
            assert Fraction(total, n) < top, "no unitig with the highest mean is cut"
    kept = {}
    for u, (s, n, total, _) in enumerate(units):
        k = len(s) - n + 1
        nodes = [m.canon(s[j:j + k]) for j in range(n)]
        assert total == sum(table[c] for c in nodes)
        if u in gone:
            st["cut"] += 1
            st["cut_nodes"] += n
            continue
        for c in nodes:
            assert c not in kept
            kept[c] = raw.get(c, table[c])
    st["out_keys"], st["out_sum"] = len(kept), sum(kept.values())
    assert st["nodes"] == st["out_keys"] + st["cut_nodes"]
    return kept, st


def model_rounds(table, rounds, **rule):
    """(the last round's table, [the statistics of every round run]): up to `rounds` rounds, each on the
    result of the one before, stopping early after one that cuts nothing (kaarme_amd.weak_rounds; counts
    below the tables' limits, so that a kept raw count reads back as it is)"""
    stats = []
    for _ in range(rounds):
        table, st = cut(table, **rule)
        stats.append(st)
        if st["cut"] == 0:
            break
    return table, stats
