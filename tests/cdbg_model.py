"""Pure-Python model of the compacted de Bruijn graph (include/kc_api.h kc_unitig_graph*) over a
{k-mer string: T(c)} dict of canonical k-mers, built on unitig_model.unitigs and
graph_model.edge_info: the unitigs and the edges between them.

A unitig U with string S_U has the orientations U+ = S_U and U- = rc(S_U); a palindromic unitig
(S_U == rc(S_U): one node that is its own reverse complement, even k only) has one, written +.  A
unitig end is a pair (node c, side s) with link(c, s) false, side L of a palindromic node aside; an
edge is reported once per set edge bit of a unitig end: (from, from_rev, to, to_rev) with from and to
indices into the unitig list.  The model asserts the header's properties on every input."""
import graph_model as m
import unitig_model as um

SIDE_BIT = {"R": m.LINK_R, "L": m.LINK_L}


def orient(string, rev):
    return m.rc(string) if rev else string


def cdbg(table, min_count=1, max_count=0, units=None):
    """(units, edges, stats): units as unitig_model.unitigs gives them ([(string, n_nodes, count_sum,
    circular)]; pass them when they are at hand), edges a list of (from, from_rev, to, to_rev), stats
    the kc_cdbg_stats dict"""
    units = um.unitigs(table, min_count, max_count) if units is None else units
    flags, gst = m.graph(table, min_count, max_count)
    nodes = set(flags)
    k = len(next(iter(nodes))) if nodes else 0
    # every node lies in one unitig: node -> (unitig, its reading inside the unitig's string)
    where = {}
    for i, (s, n, _, _) in enumerate(units):
        for j in range(n):
            x = s[j:j + k]
            assert m.canon(x) not in where
            where[m.canon(x)] = (i, x)
    assert set(where) == nodes
    pal_unit = [s == m.rc(s) for s, _, _, _ in units]
    edges, dead_ends, pal_left = [], 0, 0
    both = m.LINK_R | m.LINK_L
    for c in sorted(nodes):
        if flags[c] & both == both:
            continue  # inside a unitig
        bits, nb = m.edge_info(nodes, c)
        pal = c == m.rc(c)
        u, x = where[c]
        assert not pal or (pal_unit[u] and units[u][1] == 1)
        for s in "RL":
            if flags[c] & SIDE_BIT[s]:
                continue  # a link, not an end
            assert not units[u][3], "a circular unitig has no ends"
            if pal and s == "L":
                pal_left += len(nb[s])  # its neighbours are the ones on side R
                continue
            dead_ends += not nb[s]
            from_rev = 0 if pal_unit[u] or (c if s == "R" else m.rc(c)) == x else 1
            for d, t in nb[s]:
                v, y = where[d]
                to_rev = 0 if pal_unit[v] or (d if t == "L" else m.rc(d)) == y else 1
                edges.append((u, from_rev, v, to_rev))
    # the properties include/kc_api.h states
    for u, fr, v, tr in edges:
        assert orient(units[u][0], fr)[len(units[u][0]) - (k - 1):] == orient(units[v][0], tr)[:k - 1], (u, fr, v, tr)
    have = set(edges)
    assert len(have) == len(edges), "the tuples are distinct"
    for u, fr, v, tr in edges:
        mirror = (v, 0 if pal_unit[v] else 1 - tr, u, 0 if pal_unit[u] else 1 - fr)
        assert mirror in have, (u, fr, v, tr)
    assert len(edges) == gst["edge_ends"] - gst["link_ends"] - pal_left
    st = um.stats(units, k)
    st["edges"], st["dead_ends"] = len(edges), dead_ends
    # an open unitig has two ends, a palindromic one one
    assert sum(2 - p for p, un in zip(pal_unit, units) if not un[3]) >= dead_ends
    return units, edges, st


def palindromic_left_ends(table, min_count=1, max_count=0):
    """the edge ends on side L of palindromic nodes: edges == edge_ends - link_ends - this"""
    nodes = m.node_set(table, min_count, max_count)
    return sum(len(m.edge_info(nodes, c)[1]["L"]) for c in nodes if c == m.rc(c))


def normalised_edges(units, edges):
    """sorted [(normal of from, from_rev, normal of to, to_rev)]: a unitig is named by um.normal and
    each orientation bit is xored with "the string is not its normal form" (a palindrome never), so
    that the device's list and the model's compare whatever the strand and the order.  Unitig
    strings are distinct keys: every node lies in one unitig."""
    name, flip = [], []
    for s, n, _, circ in units:
        nm = um.normal(s, n, circ)
        name.append(nm)
        flip.append(0 if circ or s == m.rc(s) else int(s != nm))
    assert len(set(name)) == len(name)
    return sorted((name[u], fr ^ flip[u], name[v], tr ^ flip[v]) for u, fr, v, tr in edges)


def edge_tuples(edges):
    """an EDGE_DTYPE array (kaarme_amd) as the model's tuples; every other flag bit and the reserved word are 0"""
    out = []
    for a, b, fl, r in zip(edges["from"].tolist(), edges["to"].tolist(), edges["flags"].tolist(), edges["reserved"].tolist()):
        assert fl & ~3 == 0 and r == 0, (a, b, fl, r)
        out.append((a, fl & 1, b, fl >> 1 & 1))
    return out
