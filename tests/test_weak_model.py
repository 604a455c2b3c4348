"""CPU: the weak-link model (weak_model.py) on hand-built graphs (weak_cases.py, clean_cases.py,
bubble_cases.py) -- the model is what the GPU tests compare with, so its own answers are checked here
against answers worked out by hand."""
import pytest

import bubble_cases as bc
import cdbg_model as cm
import clean_cases as cc
import clean_model as clm
import graph_model as g
import weak_cases as wc
import weak_model as wm
from test_unitig_model import table_of

K = 15


def nodes_of(seq, k=K):
    return {g.canon(seq[i:i + k]) for i in range(len(seq) - k + 1)}


def unit_of(units, seq, k):
    """the index of the unitig whose nodes are the sequence's k-mers"""
    want = nodes_of(seq, k)
    (u,) = [i for i, (s, n, _, _) in enumerate(units) if nodes_of(s, k) == want]
    return u


def stats(unitigs, nodes, interior, weak, cut, cut_nodes, out_sum):
    return dict(zip(wm.FIELDS, (unitigs, nodes, interior, weak, cut, cut_nodes, nodes - cut_nodes, out_sum)))


@pytest.mark.parametrize("k", [15, 31, 32, 63, 65, 479])
def test_chimera_is_cut_and_leaves_two_unitigs(k):
    seqs, j = wc.chimera(k)
    g1, g2 = seqs[0], seqs[10]
    table = table_of(seqs, k)
    junction = nodes_of(j, k)
    assert len(junction) == k - 1 and all(table[c] == 1 for c in junction) and len(table) == 200 + k - 1
    graph = cm.cdbg(table)
    units, edges, _ = graph
    u = unit_of(units, j, k)
    assert len(units) == 5 and wm.interior(units, edges) == {u}
    assert sorted(units[v][1] for v in wm.neighbours(units, edges)[u]) == [50, 50]
    kept, st = wm.cut(table, graph=graph, max_nodes=k, ratio_permille=200)
    assert set(table) - set(kept) == junction
    assert st == stats(5, 200 + k - 1, 1, 1, 1, k - 1, 2000)
    assert sorted((n, circ) for _, n, _, circ in cm.cdbg(kept)[0]) == [(100, False), (100, False)]
    assert nodes_of(g1, k) | nodes_of(g2, k) == set(kept)
    # one node too few, the rule off, the guard below the joint's mean 1: it stays, and is still weak
    for rule in (dict(max_nodes=k - 2, ratio_permille=200), dict(), dict(ratio_permille=200)):
        kept, st = wm.cut(table, graph=graph, **rule)
        assert kept == table and (st["interior"], st["weak"], st["cut"]) == (1, 1, 0)
    # no relative test: the guard alone decides
    assert wm.cut(table, graph=graph, max_nodes=k, max_mean=1)[1]["cut"] == 1
    # from 2 on the joint is no node
    kept, st = wm.cut(table, 2, 0, max_nodes=k, ratio_permille=200)
    assert st == stats(2, 200, 0, 0, 0, 0, 2000) and set(kept) == set(table) - junction


def test_threshold_is_strict():
    """mean 2 among neighbours of mean 10: the two sides are equal at 200 per mille"""
    seqs, j = wc.chimera(K, light=2)
    table = table_of(seqs, K)
    graph = cm.cdbg(table)
    units, edges, _ = graph
    u = unit_of(units, j, K)
    s, n = wm.local(units, wm.neighbours(units, edges)[u])
    assert units[u][2] == 2 * units[u][1] and s == 10 * n and units[u][2] * n * 1000 == 200 * s * units[u][1]
    kept, st = wm.cut(table, graph=graph, max_nodes=K, ratio_permille=200)
    assert kept == table and (st["interior"], st["weak"], st["cut"]) == (1, 0, 0)
    kept, st = wm.cut(table, graph=graph, max_nodes=K, ratio_permille=201)
    assert set(table) - set(kept) == nodes_of(j) and (st["weak"], st["cut"], st["cut_nodes"]) == (1, 1, K - 1)


def test_het_bubble_loses_both_arms_at_a_high_ratio():
    """the documented hazard"""
    seqs, q = wc.het_bubble(K)
    table = table_of(seqs, K)
    graph = cm.cdbg(table)
    units, edges, _ = graph
    arms = wm.interior(units, edges)
    assert len(units) == 4 and len(arms) == 2 and all(units[u][1:3] == (K, 5 * K) for u in arms)
    assert all(units[u][2] == 10 * units[u][1] for u in range(4) if u not in arms)
    kept, st = wm.cut(table, graph=graph, max_nodes=K, ratio_permille=200)
    assert kept == table and (st["interior"], st["weak"], st["cut"]) == (2, 0, 0)
    assert wm.cut(table, graph=graph, max_nodes=K, ratio_permille=500)[1]["weak"] == 0  # 5 is not below half of 10
    kept, st = wm.cut(table, graph=graph, max_nodes=K, ratio_permille=600)
    assert (st["weak"], st["cut"], st["cut_nodes"]) == (2, 2, 2 * K) and len(cm.cdbg(kept)[0]) == 2


def double_neighbour_claims(table, graph, b, v, w, k):
    """the bridge's unitig, and that N(bridge) is {V, V, W} with a verdict that a set would not give"""
    units, edges, _ = graph
    u, uv, uw = unit_of(units, b, k), unit_of(units, v, k), unit_of(units, w, k)
    entries = wm.neighbours(units, edges)[u]
    assert sorted(entries) == sorted([uv, uv, uw]) and u in wm.interior(units, edges)
    as_multiset, as_set = wm.local(units, entries), wm.local(units, set(entries))
    assert wm.is_weak(units[u], *as_multiset, entries, 300) and not wm.is_weak(units[u], *as_set, entries, 300)
    return u


def test_a_neighbour_reached_twice_counts_twice():
    seqs, b, v, w = wc.double_neighbour(K)
    table = table_of(seqs, K)
    graph = cm.cdbg(table)
    double_neighbour_claims(table, graph, b, v, w, K)
    kept, st = wm.cut(table, graph=graph, max_nodes=2 * K, ratio_permille=300)
    assert set(table) - set(kept) == nodes_of(b) and st["cut"] == 1


def test_edges_back_into_the_unitig_give_no_entry():
    k = 31
    # poly-A: both ends lead only into itself; the hairpin is a tip, the CA circle is circular
    table = table_of(wc.SELF_LOOPS, k)
    graph = cm.cdbg(table)
    units, edges, _ = graph
    a = unit_of(units, "A" * k, k)
    assert wm.interior(units, edges) == {a} and clm.end_degrees(units, edges)[a] == (1, 1)
    assert wm.neighbours(units, edges)[a] == []
    kept, st = wm.cut(table, graph=graph, max_nodes=1000, max_mean=1000)
    assert kept == table and (st["interior"], st["weak"], st["cut"]) == (1, 0, 0)
    # one end leads only into itself, the other into itself and on: one entry
    seqs, t = wc.loop_end(k)
    table = table_of(seqs, k)
    graph = cm.cdbg(table)
    units, edges, _ = graph
    a = unit_of(units, "A" * k, k)
    assert sorted(clm.end_degrees(units, edges)[a]) == [1, 2] and len(wm.neighbours(units, edges)[a]) == 1
    assert units[a][1:3] == (1, 10) and wm.local(units, wm.neighbours(units, edges)[a]) == (20 * 60, 60)
    assert wm.cut(table, graph=graph, max_nodes=1, ratio_permille=500)[1]["weak"] == 0
    kept, st = wm.cut(table, graph=graph, max_nodes=1, ratio_permille=501)
    assert set(table) - set(kept) == {"A" * k} and (st["interior"], st["cut"]) == (1, 1)


def palindrome_claims(table, graph, p, x_unit, k):
    """P is one palindromic unitig with edges, light enough to be weak if it were interior; X's unitig
    is interior, has P among its three neighbours, and is weak at 1000 per mille only without it"""
    units, edges, _ = graph
    u, ux = unit_of(units, p, k), unit_of(units, x_unit, k)
    inside, nb = wm.interior(units, edges), wm.neighbours(units, edges)
    assert p == g.rc(p) and units[u][1] == 1 and min(clm.end_degrees(units, edges)[u]) >= 1 and u not in inside
    assert wm.is_weak(units[u], *wm.local(units, nb[u]), nb[u], 500)
    assert ux in inside and len(nb[ux]) == 3 and nb[ux].count(u) == 1
    others = [v for v in nb[ux] if v != u]
    assert not wm.is_weak(units[ux], *wm.local(units, nb[ux]), nb[ux], 1000)
    assert wm.is_weak(units[ux], *wm.local(units, others), others, 1000)
    return u, ux


def test_palindromic_unitig_is_kept_and_counts_as_a_neighbour():
    k = 32
    seqs, p, x_unit = wc.palindrome(k)
    table = table_of(seqs, k)
    graph = cm.cdbg(table)
    palindrome_claims(table, graph, p, x_unit, k)
    kept, st = wm.cut(table, graph=graph, max_nodes=1000, ratio_permille=1000)
    assert p in kept and nodes_of(x_unit, k) <= set(kept)


def test_big_counts_need_more_than_32_bits():
    seqs, j, f, ratio = wc.big_counts()
    k = 31
    table = {c: t * f for c, t in table_of(seqs, k).items()}
    assert max(table.values()) == 10 * f < 65536
    graph = cm.cdbg(table)
    units, edges, _ = graph
    u = unit_of(units, j, k)
    s, n = wm.local(units, wm.neighbours(units, edges)[u])
    lhs, rhs = units[u][2] * n * 1000, ratio * s * units[u][1]
    assert lhs >= 1 << 32 and lhs < rhs and not (lhs & 0xFFFFFFFF < rhs & 0xFFFFFFFF)
    assert max(lhs, rhs) < 1 << 64  # (what a graph of this size can reach)
    kept, st = wm.cut(table, graph=graph, max_nodes=k, ratio_permille=ratio)
    assert st["cut"] == 1 and set(table) - set(kept) == nodes_of(j, k)


def test_what_is_no_weak_link_stays():
    """tips, isolated unitigs, circles: whatever their counts"""
    for seqs in (cc.two_tip_junction(K)[0], cc.cascade(K)[0], cc.small_circle(K)[0], cc.chain_with_branch(K)[0],
                 cc.isolated_chain(K)[0]):
        table = table_of(seqs, K)
        kept, st = wm.cut(table, max_nodes=1000, ratio_permille=1000, max_mean=1000)
        assert st["cut"] == 0 and kept == table


def test_rounds_stop_when_nothing_is_cut():
    seqs, j = wc.chimera(K)
    table = table_of(seqs, K)
    last, per_round = wm.model_rounds(table, 5, max_nodes=K, ratio_permille=200)
    assert [s["cut"] for s in per_round] == [1, 0] and per_round[1]["unitigs"] == 2 and len(last) == 200
    last1, per_round1 = wm.model_rounds(table, 1, max_nodes=K, ratio_permille=200)
    assert last1 == last and per_round1 == per_round[:1]


@pytest.mark.parametrize("k,length,sites,seeds", [(6, 150, 10, 30), (8, 400, 20, 5)])
def test_dense_small_k_invariants(k, length, sites, seeds):
    """accidental repeats, self loops and (even k) palindromic nodes: the model's own assertions on every
    rule, and something is cut"""
    cut = 0
    for seed in range(seeds):
        table = table_of(bc.dense(k, seed, length, sites), k)
        for lo in (1, 2):
            in_range = {c for c, t in table.items() if t >= lo}
            graph = cm.cdbg(table, lo, 0)
            for rule in (dict(), dict(max_nodes=k, ratio_permille=200), dict(max_nodes=2 * k, ratio_permille=1000),
                         dict(max_nodes=3 * k, max_mean=1), dict(max_nodes=3 * k, ratio_permille=600, max_mean=2)):
                kept, st = wm.cut(table, lo, 0, graph=graph, **rule)
                assert set(kept) <= in_range and st["nodes"] == len(in_range) and all(kept[c] == table[c] for c in kept)
                if not rule:
                    assert kept == {c: table[c] for c in in_range}
                cut += st["cut"]
    assert cut > 0


def test_read_errors_invariants():
    """the invariants on a graph of reads with substitutions (test_gpu_graph.make_reads, a genome of 3000
    bases and 300 reads)"""
    from test_gpu_graph import make_reads
    data = make_reads(3, n_reads=300, genome_len=3000)
    reads = [line.decode() for line in data.split(b"\n") if line and not line.startswith(b">")]
    table = table_of(reads, K)
    graph = cm.cdbg(table)
    for rule in (dict(max_nodes=K, ratio_permille=200), dict(max_nodes=2 * K, ratio_permille=1000), dict(max_nodes=K, max_mean=1)):
        kept, st = wm.cut(table, graph=graph, **rule)
        assert st["interior"] >= st["weak"] >= st["cut"] > 0
