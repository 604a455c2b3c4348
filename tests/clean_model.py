"""Pure-Python model of graph cleaning (include/kc_api.h kc_clean*) over a {k-mer string: T(c)} dict
of canonical k-mers, built on cdbg_model.cdbg: the unitigs of the range's graph and the edges between
them.

For unitig u the edges with from == u are the set edge bits of its ends, and from_rev tells the end:
0 the end of its string, 1 the start.  The degree of an end is the number of those edges.  A
palindromic unitig (one node, its own reverse complement) reports its edges once, with from_rev 0,
and its side-L neighbours are its side-R neighbours complemented: both ends have that one degree.
  isolated   open, both ends of degree 0
  tip        open, exactly one end of degree 0
  guard      max_mean != 0: removable only when count_sum <= max_mean * n_nodes
  removed    a tip with tip_max_nodes != 0 and n_nodes <= tip_max_nodes, or an isolated unitig with
             iso_max_nodes != 0 and n_nodes <= iso_max_nodes, the guard passing
Every verdict is taken on the one graph, so no order matters; the nodes of every other unitig are
kept with their raw counts."""
import cdbg_model as cm
import graph_model as m

FIELDS = ("unitigs", "nodes", "tips", "tip_nodes", "isolated", "isolated_nodes", "out_keys", "out_sum")


def end_degrees(units, edges):
    """[(degree of the string's end, degree of its start)] per unitig"""
    deg = [[0, 0] for _ in units]
    for u, from_rev, _, _ in edges:
        deg[u][from_rev] += 1
    for u, (s, n, _, _) in enumerate(units):
        if s == m.rc(s):  # palindromic: side L mirrors side R
            assert n == 1 and deg[u][1] == 0
            deg[u][1] = deg[u][0]
    return [tuple(d) for d in deg]


def category(unit, degrees):
    """'isolated', 'tip' or None of one unitig"""
    if unit[3]:
        return None
    dead = sum(d == 0 for d in degrees)
    return "isolated" if dead == 2 else "tip" if dead == 1 else None


def clean(table, min_count=1, max_count=0, tip_max_nodes=0, iso_max_nodes=0, max_mean=0, raw=None, graph=None):
    """(kept {k-mer: raw count}, the kc_clean_stats dict).  table holds T(c); raw (default: none
    differs) the raw counts of the k-mers whose raw count is not their T(c); graph: cdbg_model.cdbg
    of the same table and range, when it is at hand."""
    units, edges, cst = graph or cm.cdbg(table, min_count, max_count)
    raw = raw or {}
    st = dict.fromkeys(FIELDS, 0)
    st["unitigs"], st["nodes"] = cst["unitigs"], cst["nodes"]
    kept = {}
    for unit, degrees in zip(units, end_degrees(units, edges)):
        s, n, total, _ = unit
        k = len(s) - n + 1
        nodes = [m.canon(s[j:j + k]) for j in range(n)]
        assert total == sum(table[c] for c in nodes)
        cat = category(unit, degrees)
        assert not (s == m.rc(s) and cat == "tip"), "a palindromic unitig is never a tip"
        limit = {"tip": tip_max_nodes, "isolated": iso_max_nodes, None: 0}[cat]
        guard = max_mean == 0 or total <= max_mean * n
        if limit and n <= limit and guard:
            st["tips" if cat == "tip" else "isolated"] += 1
            st["tip_nodes" if cat == "tip" else "isolated_nodes"] += n
            continue
        for c in nodes:
            assert c not in kept
            kept[c] = raw.get(c, table[c])
    st["out_keys"], st["out_sum"] = len(kept), sum(kept.values())
    assert st["nodes"] == st["out_keys"] + st["tip_nodes"] + st["isolated_nodes"]
    return kept, st


def model_rounds(table, rounds, **rule):
    """(the last round's table, [the statistics of every round run]): up to `rounds` rounds, each on the
    result of the one before, stopping early after one that removes nothing (kaarme_amd.clean_rounds;
    counts below the tables' limits, so that a kept raw count reads back as it is)"""
    stats = []
    for _ in range(rounds):
        table, st = clean(table, **rule)
        stats.append(st)
        if st["tips"] == 0 and st["isolated"] == 0:
            break
    return table, stats
