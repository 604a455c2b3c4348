"""Pure-Python model of the de Bruijn graph layer (include/kc_api.h kc_neighbors*, kc_graph*) over a
{k-mer string: T(c)} dict of canonical k-mers -- what decode_records(dump()) gives.

Strings are over ACGT; rc is the reverse complement, canon(z) = min(z, rc(z)).  A range is min_count
(0 means 1) and max_count (0 = no upper bound).
  node        a canonical k-mer c of the dict with min_count <= T(c) <= max_count
  edges of c  bit y: canon(c[1:] + y) is a node (side R); bit 4 + y: canon(y + c[:-1]) is a node (L)
  facing      side R, z = c[1:] + y, d = canon(z): c sits on d's side L if d == z, else on d's R;
              side L, z = y + c[:-1]: on d's side R if d == z, else on d's side L
  link(c, s)  deg_s(c) == 1, its one neighbour d != c, neither c nor d is its own reverse complement,
              and the degree of d's facing side is 1
  flags       bits 0-7 the edges, LINK_R, LINK_L, NODE"""
_COMP = str.maketrans("ACGT", "TGCA")
BASES = "ACGT"
LINK_R, LINK_L, NODE = 0x100, 0x200, 0x8000
FIELDS = ("nodes", "edge_ends", "link_ends", "isolated", "palindromes")  # then side_degree[5]


def rc(s):
    return s.translate(_COMP)[::-1]


def canon(s):
    return min(s, rc(s))


def in_range(t, min_count=1, max_count=0):
    return t >= (min_count or 1) and (max_count == 0 or t <= max_count)


def node_set(table, min_count=1, max_count=0):
    return {c for c, t in table.items() if in_range(t, min_count, max_count)}


def neighbor_strings(x):
    """the eight neighbours of x as read: x[1:] + y for y in ACGT, then y + x[:-1]"""
    return [x[1:] + y for y in BASES] + [y + x[:-1] for y in BASES]


def neighbors(table, x):
    """kc_neighbors of the k-mer x (either strand, as given): T of its eight neighbours"""
    return [table.get(canon(z), 0) for z in neighbor_strings(x)]


def edge_info(nodes, c):
    """(edge bits, {side: [(neighbour, the side of it c sits on)]}) of node c; sides 'R' and 'L'"""
    bits, nb = 0, {"R": [], "L": []}
    for i, z in enumerate(neighbor_strings(c)):
        d = canon(z)
        if d not in nodes:
            continue
        bits |= 1 << i
        if i < 4:
            nb["R"].append((d, "L" if d == z else "R"))
        else:
            nb["L"].append((d, "R" if d == z else "L"))
    return bits, nb


def graph(table, min_count=1, max_count=0):
    """({node: flags}, statistics) -- kc_graph's records as a dict and its kc_graph_stats, with
    side_degree as a list and open_unitigs = nodes - link_ends / 2 (KmerCounter.graph's dict)"""
    nodes = node_set(table, min_count, max_count)
    info = {c: edge_info(nodes, c) for c in nodes}
    flags = {}
    st = dict.fromkeys(FIELDS, 0)
    st["side_degree"] = [0] * 5
    for c in nodes:
        bits, nb = info[c]
        f = bits | NODE
        for s, bit in (("R", LINK_R), ("L", LINK_L)):
            st["side_degree"][len(nb[s])] += 1
            if len(nb[s]) != 1:
                continue
            d, t = nb[s][0]
            if d == c or c == rc(c) or d == rc(d):
                continue
            if len(info[d][1][t]) == 1:
                f |= bit
        flags[c] = f
        st["nodes"] += 1
        st["edge_ends"] += bin(bits).count("1")
        st["link_ends"] += bin(f & (LINK_R | LINK_L)).count("1")
        st["isolated"] += bits == 0
        st["palindromes"] += c == rc(c)
    st["open_unitigs"] = st["nodes"] - st["link_ends"] // 2
    return flags, st


def link_partner(nodes, c, s):
    """(d, t): the node and side a set link bit of (c, s) leads to"""
    (d, t), = edge_info(nodes, c)[1][s]
    return d, t


def node_line(c, t, flags):
    """the CLI's --graph line of a node"""
    r = "".join(b if flags >> i & 1 else "." for i, b in enumerate(BASES))
    l = "".join(b if flags >> (4 + i) & 1 else "." for i, b in enumerate(BASES))
    links = ("L" if flags & LINK_L else "-") + ("R" if flags & LINK_R else "-")
    return f"{c} {t} {r} {l} {links}"
