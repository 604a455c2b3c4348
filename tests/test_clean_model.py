"""CPU: the graph-cleaning model (clean_model.py) on hand-built graphs (clean_cases.py) -- the model is
what the GPU tests compare with, so its own answers are checked here against answers worked out by
hand."""
import numpy as np

import cdbg_model as cm
import clean_cases as cc
import clean_model as clm
import graph_model as g
from test_unitig_model import table_of

K = 15


def nodes_of(seq, k=K):
    return {g.canon(seq[i:i + k]) for i in range(len(seq) - k + 1)}


def shape(table, lo=1, hi=0):
    """sorted [(n_nodes, category or "-")] of the range's unitigs"""
    units, edges, _ = cm.cdbg(table, lo, hi)
    return sorted((u[1], clm.category(u, d) or "-") for u, d in zip(units, clm.end_degrees(units, edges)))


def stats(unitigs, nodes, tips=0, tip_nodes=0, isolated=0, isolated_nodes=0, out_sum=None):
    out = nodes - tip_nodes - isolated_nodes
    return dict(zip(clm.FIELDS, (unitigs, nodes, tips, tip_nodes, isolated, isolated_nodes, out, out if out_sum is None else out_sum)))


def test_chain_with_one_branch():
    seqs, b = cc.chain_with_branch(K)
    table = table_of(seqs, K)
    # the genome's two pieces are tips too: a dead end and a junction each, but 40 and 50 nodes long
    assert shape(table) == [(3, "tip"), (40, "tip"), (50, "tip")]
    kept, st = clm.clean(table, tip_max_nodes=2)
    assert kept == table and st == stats(3, 93, out_sum=sum(table.values()))
    kept, st = clm.clean(table, tip_max_nodes=3)
    gone = nodes_of(b) - nodes_of(seqs[0])
    assert len(gone) == 3 and kept == {c: t for c, t in table.items() if c not in gone}
    assert st == stats(3, 93, 1, 3, out_sum=sum(kept.values()))
    assert kept == table_of(seqs[:1], K)  # what is left is the genome, one chain
    assert shape(kept) == [(90, "isolated")]
    # the isolated rule alone removes nothing here
    assert clm.clean(table, iso_max_nodes=1000)[0] == table


def test_guard_keeps_a_heavy_tip():
    seqs, b = cc.chain_with_branch(K, heavy=10)
    table = table_of(seqs, K)
    gone = nodes_of(b) - nodes_of(seqs[0])
    assert all(table[c] == 10 for c in gone) and len(gone) == 3
    for max_mean, removed in ((0, True), (9, False), (10, True), (5, False)):  # count_sum 30 <= max_mean * 3
        kept, st = clm.clean(table, tip_max_nodes=3, max_mean=max_mean)
        assert (st["tips"], st["tip_nodes"]) == ((1, 3) if removed else (0, 0)), max_mean
        assert (set(table) - set(kept) == gone) if removed else kept == table


def test_isolated_chain():
    seqs, c = cc.isolated_chain(K)
    table = table_of(seqs, K)
    assert shape(table) == [(5, "isolated"), (60, "isolated")]
    kept, st = clm.clean(table, iso_max_nodes=4)
    assert kept == table and st == stats(2, 65)
    kept, st = clm.clean(table, iso_max_nodes=5)
    assert kept == table_of(seqs[:1], K) and st == stats(2, 65, isolated=1, isolated_nodes=5)
    assert clm.clean(table, iso_max_nodes=60)[1] == stats(2, 65, isolated=2, isolated_nodes=65)
    assert clm.clean(table, tip_max_nodes=1000)[0] == table  # no tips here


def test_circle_is_never_removed():
    seqs, c = cc.small_circle(K)
    table = table_of(seqs, K)
    units, _, _ = cm.cdbg(table)
    assert sorted((u[1], u[3]) for u in units) == [(5, True), (60, False)]
    assert shape(table) == [(5, "-"), (60, "isolated")]
    kept, st = clm.clean(table, tip_max_nodes=1000, iso_max_nodes=1000)
    assert set(kept) == nodes_of(seqs[1]) and len(kept) == 5
    assert st == stats(2, 65, isolated=1, isolated_nodes=60, out_sum=sum(kept.values()))


def test_bubble_keeps_both_arms():
    seqs, q = cc.bubble(K)
    table = table_of(seqs, K)
    # the genome before and after the bubble (tips of 50 and 35 nodes) and the two arms of K nodes
    assert shape(table) == [(K, "-"), (K, "-"), (100 - 50 - K, "tip"), (50, "tip")]
    kept, st = clm.clean(table, tip_max_nodes=K, iso_max_nodes=K)
    assert kept == table and st == stats(4, 100 + K)


def test_junction_of_two_short_tips_loses_both():
    seqs, stem = cc.two_tip_junction(K)
    table = table_of(seqs, K)
    assert shape(table) == [(3, "tip"), (3, "tip"), (50, "tip")]
    kept, st = clm.clean(table, tip_max_nodes=3)
    assert kept == dict.fromkeys(table_of([stem], K), 2) and st == stats(3, 56, 2, 6, out_sum=50 * 2)


def test_cascade_takes_three_rounds():
    n = 3
    seqs, b, c = cc.cascade(K, n=n)
    table = table_of(seqs, K)
    # genome 40 + 50, B's near piece between two junctions, its far piece and the sub-branch
    assert shape(table) == [(n, "-"), (n, "tip"), (n, "tip"), (40, "tip"), (50, "tip")]
    near = {g.canon(b[i:i + K]) for i in range(n)}
    far = {g.canon(b[i:i + K]) for i in range(n, 2 * n)}
    sub = nodes_of(c) - nodes_of(b)
    assert len(near) == len(far) == len(sub) == n
    kept1, st1 = clm.clean(table, tip_max_nodes=n)
    assert set(table) - set(kept1) == far | sub and st1 == stats(5, 90 + 3 * n, 2, 2 * n, out_sum=sum(kept1.values()))
    kept2, st2 = clm.clean(kept1, tip_max_nodes=n)
    assert set(kept1) - set(kept2) == near and st2 == stats(3, 90 + n, 1, n, out_sum=sum(kept2.values()))
    kept3, st3 = clm.clean(kept2, tip_max_nodes=n)
    assert kept3 == kept2 and st3 == stats(1, 90, out_sum=sum(kept2.values())) and set(kept3) == nodes_of(seqs[0])
    last, per_round = clm.model_rounds(table, 5, tip_max_nodes=n)
    assert last == kept3 and per_round == [st1, st2, st3]
    last, per_round = clm.model_rounds(table, 2, tip_max_nodes=n)
    assert last == kept2 and per_round == [st1, st2]


def test_dense_k4_invariants():
    """palindromic nodes with neighbours, self loops, sides of degree 4: the model's own assertions (the
    node balance, no palindromic tip, every node kept once) on every rule and range"""
    k = 4
    rng = np.random.default_rng(204)
    table = table_of([cc.rand(rng, 300)], k)
    nodes = set(table)
    pals = [c for c in nodes if c == g.rc(c)]
    assert any(g.edge_info(nodes, c)[0] for c in pals)
    med = int(np.median(list(table.values())))
    seen_removal = False
    for lo, hi in ((1, 0), (med, 0), (1, med), (med + 1, 0)):
        in_range = {c for c, t in table.items() if g.in_range(t, lo, hi)}
        for rule in (dict(), dict(tip_max_nodes=3), dict(iso_max_nodes=3), dict(tip_max_nodes=3, iso_max_nodes=3),
                     dict(tip_max_nodes=100, iso_max_nodes=100, max_mean=med)):
            kept, st = clm.clean(table, lo, hi, **rule)
            assert set(kept) <= in_range and st["nodes"] == len(in_range)
            assert all(kept[c] == table[c] for c in kept)
            if not rule:
                assert set(kept) == in_range
            seen_removal |= st["tips"] + st["isolated"] > 0
    assert seen_removal
