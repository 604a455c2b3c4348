"""Pure-Python model of bubble popping (include/kc_api.h kc_pop_bubbles*) over a {k-mer string: T(c)}
dict of canonical k-mers, built on cdbg_model.cdbg: the unitigs of the range's graph and the edges
between them.

  branch    U is open and not palindromic, both ends have degree exactly 1, neither edge leads to U
  anchor    for the edge (U, from_rev, V, to_rev): (V, 1 - to_rev), (V, 1) for a palindromic V; a
            branch has two, and they differ
  parallel  two different branches with the same unordered pair of anchors
  beats     U' beats U: count_sum(U') * n(U) > count_sum(U) * n(U'), or equal and name(U') < name(U);
            name: the smaller of the canonical k-mers of the two end nodes
  popped    max_nodes != 0, n(U) <= max_nodes, the guard passes, and some parallel U' with n(U') <=
            max_nodes and |n(U) - n(U')| <= max_diff beats U
Every verdict is taken on the one graph; the nodes of every other unitig are kept with their raw
counts.  The model asserts the node balance, that no anchor is popped and that every set of parallel
branches keeps at least one, on every input."""
import cdbg_model as cm
import graph_model as m

FIELDS = ("unitigs", "nodes", "branches", "parallel", "popped", "popped_nodes", "out_keys", "out_sum")


def name(unit):
    s, n, _, _ = unit
    k = len(s) - n + 1
    return min(m.canon(s[:k]), m.canon(s[-k:]))


def branches(units, edges):
    """{unitig index: frozenset of its two anchors} of the branches"""
    pal = [s == m.rc(s) for s, _, _, _ in units]
    out_edges = [[[], []] for _ in units]
    for u, fr, v, tr in edges:
        out_edges[u][fr].append((v, tr))
    out = {}
    for u, (s, n, _, circ) in enumerate(units):
        if circ or pal[u]:
            continue
        e0, e1 = out_edges[u]
        if len(e0) != 1 or len(e1) != 1 or e0[0][0] == u or e1[0][0] == u:
            continue
        anchors = frozenset((v, 1 if pal[v] else 1 - tr) for v, tr in (e0[0], e1[0]))
        if len(anchors) == 2:
            out[u] = anchors
    return out


def beats(a, b):
    """unit a beats unit b"""
    pa, pb = a[2] * b[1], b[2] * a[1]
    return pa > pb or (pa == pb and name(a) < name(b))


def pop(table, min_count=1, max_count=0, max_nodes=0, max_diff=0, max_mean=0, raw=None, graph=None):
    """(kept {k-mer: raw count}, the kc_bubble_stats dict).  table holds T(c); raw (default: none
    differs) the raw counts of the k-mers whose raw count is not their T(c); graph: cdbg_model.cdbg
    of the same table and range, when it is at hand."""
    units, edges, cst = graph or cm.cdbg(table, min_count, max_count)
    raw = raw or {}
    st = dict.fromkeys(FIELDS, 0)
    st["unitigs"], st["nodes"] = cst["unitigs"], cst["nodes"]
    br = branches(units, edges)
    st["branches"] = len(br)
    sets = {}
    for u, anchors in br.items():
        sets.setdefault(anchors, []).append(u)
    assert len({name(u) for u in units}) == len(units), "distinct unitigs have distinct names"
    popped = set()
    for anchors, members in sets.items():
        assert len(members) <= 4, "at most four branches share an anchor end"
        if len(members) < 2:
            continue
        st["parallel"] += len(members)
        for u in members:
            s, n, total, _ = units[u]
            if not (max_nodes and n <= max_nodes and (max_mean == 0 or total <= max_mean * n)):
                continue
            if any(v != u and units[v][1] <= max_nodes and abs(units[v][1] - n) <= max_diff and beats(units[v], units[u])
                   for v in members):
                popped.add(u)
        assert any(u not in popped for u in members), "every set of parallel branches keeps at least one"
        top = [u for u in members if not any(beats(units[v], units[u]) for v in members if v != u)]
        assert len(top) == 1 and top[0] not in popped, "the one that no other beats stays"
    for anchors in br.values():
        assert not any(v in popped for v, _ in anchors), "no anchor is popped"
    kept = {}
    for u, (s, n, total, _) in enumerate(units):
        k = len(s) - n + 1
        nodes = [m.canon(s[j:j + k]) for j in range(n)]
        assert total == sum(table[c] for c in nodes)
        if u in popped:
            st["popped"] += 1
            st["popped_nodes"] += n
            continue
        for c in nodes:
            assert c not in kept
            kept[c] = raw.get(c, table[c])
    st["out_keys"], st["out_sum"] = len(kept), sum(kept.values())
    assert st["nodes"] == st["out_keys"] + st["popped_nodes"]
    return kept, st


def model_rounds(table, rounds, **rule):
    """(the last round's table, [the statistics of every round run]): up to `rounds` rounds, each on the
    result of the one before, stopping early after one that pops nothing (kaarme_amd.pop_rounds; counts
    below the tables' limits, so that a kept raw count reads back as it is)"""
    stats = []
    for _ in range(rounds):
        table, st = pop(table, **rule)
        stats.append(st)
        if st["popped"] == 0:
            break
    return table, stats
