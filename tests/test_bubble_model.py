"""CPU: the bubble-popping model (bubble_model.py) on hand-built graphs (bubble_cases.py, clean_cases.py)
-- the model is what the GPU tests compare with, so its own answers are checked here against answers
worked out by hand."""
import numpy as np
import pytest

import bubble_cases as bc
import bubble_model as bm
import cdbg_model as cm
import clean_cases as cc
import graph_model as g
from test_unitig_model import table_of

K = 15


def nodes_of(seq, k=K):
    return {g.canon(seq[i:i + k]) for i in range(len(seq) - k + 1)}


def parallel_sets(graph):
    """sorted sizes of the sets of mutually parallel branches of cm.cdbg's graph"""
    units, edges, _ = graph
    sets = {}
    for u, anchors in bm.branches(units, edges).items():
        sets[anchors] = sets.get(anchors, 0) + 1
    return sorted(n for n in sets.values() if n > 1)


def test_bubble_loses_the_substituted_arm():
    seqs, q = cc.bubble(K)
    g0, alt = seqs
    arm_alt, arm_g = nodes_of(alt) - nodes_of(g0), nodes_of(g0[q - K + 1:q + K])
    assert len(arm_alt) == len(arm_g) == K
    table = table_of([g0] * 3 + [alt], K)
    assert parallel_sets(cm.cdbg(table)) == [2]
    kept, st = bm.pop(table, max_nodes=K)
    assert set(table) - set(kept) == arm_alt
    assert st == dict(zip(bm.FIELDS, (4, 100 + K, 2, 2, 1, K, 100, sum(kept.values()))))
    assert kept == {c: t for c, t in table.items() if c not in arm_alt}
    # one node too few, or the rule off: both arms stay
    for max_nodes in (K - 1, 0):
        kept, st = bm.pop(table, max_nodes=max_nodes)
        assert kept == table and (st["branches"], st["parallel"], st["popped"]) == (2, 2, 0)
    # the guard: the substituted arm has mean 1
    assert bm.pop(table, max_nodes=K, max_mean=1)[1]["popped"] == 1
    # given once each, all means are equal and the name decides, whichever comes first
    once, twice = table_of([g0, alt], K), table_of([alt, g0], K)
    assert once == twice
    units, edges, _ = cm.cdbg(once)
    arms = [units[u] for u in bm.branches(units, edges)]
    assert len(arms) == 2 and arms[0][2] * arms[1][1] == arms[1][2] * arms[0][1]
    loser = max(arms, key=bm.name)
    kept, st = bm.pop(once, max_nodes=K)
    assert st["popped"] == 1 and set(once) - set(kept) == nodes_of(loser[0])


@pytest.mark.parametrize("k", [8, 15, 31, 32, 63, 65, 479])
def test_variants(k):
    seqs, alts = bc.variants(k)
    table = table_of(seqs, k)
    graph = cm.cdbg(table)
    assert len(graph[0]) == 14 and parallel_sets(graph) == [2, 2, 2, 3]
    g0 = seqs[0]
    new = {kind: set() for _, kind, _ in alts}
    for _, kind, a in alts:
        new[kind] |= nodes_of(a, k) - nodes_of(g0, k)
    assert (len(new["sub"]), len(new["sub2"]), len(new["del"])) == (2 * k, 2 * k, k - 1)
    kept, st = bm.pop(table, graph=graph, max_nodes=k, max_diff=0)
    assert (st["branches"], st["parallel"], st["popped"], st["popped_nodes"]) == (9, 9, 4, 4 * k)
    assert set(table) - set(kept) == new["sub"] | new["sub2"]
    kept, st = bm.pop(table, graph=graph, max_nodes=k, max_diff=1)
    assert (st["popped"], st["popped_nodes"]) == (5, 5 * k - 1) and set(kept) == nodes_of(g0, k)
    assert bm.pop(table, graph=graph, max_nodes=k - 1, max_diff=0)[1]["popped"] == 0
    # the deletion's arm alone is short enough, but its only parallel arm is not
    assert bm.pop(table, graph=graph, max_nodes=k - 1, max_diff=1)[1]["popped"] == 0
    # given once, every mean is 1 (the variants' first and last nodes are the genome's own): the name decides
    once = table_of(bc.variants(k, heavy=1)[0], k)
    graph = cm.cdbg(once)
    units, edges, _ = graph
    br = bm.branches(units, edges)
    assert len(br) == 9 and all(units[u][2] == units[u][1] for u in br)
    kept, st = bm.pop(once, graph=graph, max_nodes=k, max_diff=0)
    assert st["popped"] == 4
    gone = set(once) - set(kept)
    for anchors in set(br.values()):
        members = [u for u in br if br[u] == anchors and units[u][1] == k]
        stays = min(members, key=lambda u: bm.name(units[u]))
        for u in members:
            assert (nodes_of(units[u][0], k) <= gone) == (u != stays)


def test_what_is_no_bubble_stays():
    for seqs in (cc.two_tip_junction(K)[0], cc.cascade(K)[0], cc.small_circle(K)[0], cc.chain_with_branch(K)[0]):
        table = table_of(seqs, K)
        kept, st = bm.pop(table, max_nodes=1000, max_diff=1000)
        assert kept == table and (st["parallel"], st["popped"]) == (0, 0)
    # branches without a parallel one: a tip in the middle of the genome's arm cuts it into two unitigs;
    # the substituted arm and the genome arm's second piece are branches, and their anchors differ
    seqs, q = cc.bubble(K)
    tip = cc.branch(np.random.default_rng(9), seqs[0], 57, 3, K)
    table = table_of(seqs + [tip], K)
    kept, st = bm.pop(table, max_nodes=1000, max_diff=1000)
    assert kept == table and (st["unitigs"], st["branches"], st["parallel"], st["popped"]) == (6, 2, 0, 0)


def test_rounds_stop_when_nothing_is_popped():
    seqs, _ = bc.variants(K)
    table = table_of(seqs, K)
    last, per_round = bm.model_rounds(table, 5, max_nodes=K, max_diff=1)
    assert [s["popped"] for s in per_round] == [5, 0] and set(last) == nodes_of(seqs[0])
    assert per_round[1]["unitigs"] == 1
    last1, per_round1 = bm.model_rounds(table, 1, max_nodes=K, max_diff=1)
    assert last1 == last and per_round1 == per_round[:1]


def test_palindromic_anchor():
    for k in (6, 32):
        seqs, p = bc.palindromic_anchor(k)
        table = table_of(seqs, k)
        units, edges, _ = cm.cdbg(table)
        br = bm.branches(units, edges)
        pal = [u for u, un in enumerate(units) if un[0] == p]
        assert len(pal) == 1 and p == g.rc(p) and len(br) == 2 and len(set(br.values())) == 1
        assert (pal[0], 1) in next(iter(br.values()))
        kept, st = bm.pop(table, max_nodes=k)
        assert (st["parallel"], st["popped"], st["popped_nodes"]) == (2, 1, k)
        assert set(table) - set(kept) == nodes_of(seqs[2], k) - nodes_of(seqs[0], k)


@pytest.mark.parametrize("k,length,sites,seeds", [(6, 150, 10, 30), (8, 400, 20, 5)])
def test_dense_small_k_invariants(k, length, sites, seeds):
    """accidental repeats, self loops and (even k) palindromic nodes: the model's own assertions on every
    rule, and something is popped"""
    popped = 0
    for seed in range(seeds):
        table = table_of(bc.dense(k, seed, length, sites), k)
        for lo in (1, 2):
            in_range = {c for c, t in table.items() if t >= lo}
            for rule in (dict(), dict(max_nodes=k), dict(max_nodes=k, max_diff=1), dict(max_nodes=3 * k, max_diff=k, max_mean=2)):
                kept, st = bm.pop(table, lo, 0, **rule)
                assert set(kept) <= in_range and st["nodes"] == len(in_range) and all(kept[c] == table[c] for c in kept)
                if not rule:
                    assert kept == {c: table[c] for c in in_range}
                popped += st["popped"]
    assert popped > 0
