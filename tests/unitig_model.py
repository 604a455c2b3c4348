"""Pure-Python model of the unitig layer (include/kc_api.h kc_unitigs*) over a {k-mer string: T(c)}
dict of canonical k-mers, built on graph_model.graph / link_partner: a plain walk along the links.

A unitig is a maximal path of links c_0 ... c_{n-1}, each node read on one strand (x_i in {c_i,
rc(c_i)}, x_{i+1}[:-1] == x_i[1:]); its string is x_0 + the last character of each later x_i.  A
circular unitig is written from an unspecified node with the same n + k - 1 bases.  The directed
states are (node, exit side): leaving c through R reads c as it is, through L as rc(c);
next(c, s) = (d, the other side of d's facing side) when link(c, s) holds."""
from graph_model import LINK_L, LINK_R, canon, graph, link_partner, rc

OTHER = {"R": "L", "L": "R"}
BIT = {"R": LINK_R, "L": LINK_L}


def _read(c, s):
    """node c as read when it is left through side s"""
    return c if s == "R" else rc(c)


def unitigs(table, min_count=1, max_count=0):
    """[(string, n_nodes, count_sum, circular)] of the graph of the table's k-mers in the range, and
    the model's own checks of the state argument and of the totals"""
    flags, st = graph(table, min_count, max_count)
    nodes = set(flags)
    nxt = {}
    for c in nodes:
        for s in "RL":
            if flags[c] & BIT[s]:
                d, t = link_partner(nodes, c, s)
                assert d != c, "a self-link"
                nxt[c, s] = (d, OTHER[t])
    # next is injective, and rev(c, s) = (c, other side) reverses it
    assert len(set(nxt.values())) == len(nxt)
    for (c, s), (d, t) in nxt.items():
        assert nxt[d, OTHER[t]] == (c, OTHER[s])
    used, out = set(), []
    for c in sorted(nodes):
        if c in used:
            continue
        # to the far end through L (or once round the circle)
        state, circular = (c, "L"), False
        while state in nxt:
            state = nxt[state]
            if state == (c, "L"):
                circular = True
                break
        state = (c, "R") if circular else (state[0], OTHER[state[1]])
        first = state
        x = _read(*state)
        string, n, total, seen = x, 0, 0, set()
        while True:
            node = state[0]
            assert node not in used and node not in seen, "a path passes one node twice"
            seen.add(node)
            n += 1
            total += table[node]
            state = nxt.get(state)
            if state is None or state == first:
                break
            y = _read(*state)
            assert y[:-1] == x[1:]
            string += y[-1]
            x = y
        assert circular == (state == first)
        if circular:
            # x_{n-1} runs on into x_0, so the last k - 1 bases repeat the first k - 1
            assert n >= 2 and string[n:] == string[:len(c) - 1]
        used |= seen
        out.append((string, n, total, circular))
    assert used == nodes
    k = len(next(iter(nodes))) if nodes else 0
    tot = stats(out, k)
    assert tot["unitigs"] - tot["circular"] == st["open_unitigs"]
    assert tot["nodes"] == st["nodes"] and tot["bases"] == tot["nodes"] + (k - 1) * tot["unitigs"]
    return out


def stats(units, k):
    """kc_unitig_stats of a list of (string, n_nodes, count_sum, circular)"""
    return {"unitigs": len(units), "circular": sum(1 for u in units if u[3]), "nodes": sum(u[1] for u in units),
            "bases": sum(len(u[0]) for u in units), "max_nodes": max((u[1] for u in units), default=0)}


def normal(string, n, circular):
    """the one name of a unitig's two (open) or 2 n (circular) right strings"""
    if not circular:
        return canon(string)
    s = string[:n]
    return min((t + t)[i:i + n] for t in (s, rc(s)) for i in range(n))


def normalised(units):
    """sorted [(normal, n_nodes, count_sum, circular)]"""
    return sorted((normal(s, n, circ), n, total, bool(circ)) for s, n, total, circ in units)


def check_strings(units, k):
    """every (string, n_nodes, ...) has n + k - 1 bases over ACGT, a circle's last k - 1 its first"""
    for s, n, _, circ in units:
        assert len(s) == n + k - 1 and set(s) <= set("ACGT"), (s, n)
        if circ:
            assert n >= 2 and s[n:] == s[:k - 1], (s, n)
