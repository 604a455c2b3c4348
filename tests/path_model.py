"""Pure-Python model of the read paths (include/kc_api.h kc_read_paths*) over a {k-mer string: T(c)}
dict of canonical k-mers, built on unitig_model.unitigs and cdbg_model.cdbg: the place of every
node, then the runs, the joined flags and the per-sequence fields straight from the definitions.

A text is a string with offsets (sequence i is text[offsets[i]:offsets[i + 1]]); A, C, G, T in either
case are bases, every other character a break; a window never spans two sequences.  The model asserts
the header's properties on every input."""
import cdbg_model as cm
import graph_model as m

BASES = set("ACGT")


def pack(seqs):
    """(text, offsets) as kaarme_amd.pack_sequences joins sequences: one newline behind each"""
    text, offsets = "", [0]
    for s in seqs:
        text += s + "\n"
        offsets.append(len(text))
    return text, offsets


def places(units, k):
    """canonical node -> (unitig, its reading inside the unitig's string, its index there)"""
    where = {}
    for i, (s, n, _, _) in enumerate(units):
        for j in range(n):
            x = s[j:j + k]
            assert m.canon(x) not in where
            where[m.canon(x)] = (i, x, j)
    return where


def locate(units, where, w):
    """the place (U, rev, q) of the window w (k upper-case bases), or None"""
    hit = where.get(m.canon(w))
    if hit is None:
        return None
    i, x, j = hit
    s, n = units[i][0], units[i][1]
    rev = 0 if s == m.rc(s) or w == x else 1
    q = n - 1 - j if rev else j
    assert cm.orient(s, rev)[q:q + len(w)] == w, (s, rev, q, w)
    return i, rev, q


def spelled(unit, k, rev, q, windows):
    """the string of `windows` windows from q on orient(S_U, rev), round the circle if it is one"""
    s, n, _, circ = unit
    t = cm.orient(s, rev)
    if circ:
        laps = (q + windows + k - 1) // n + 2
        t = t[:n] * laps
    assert circ or q + windows <= n
    return t[q:q + windows + k - 1]


def paths(table, text, offsets, k, min_count=1, max_count=0, graph=None):
    """(units, edges, cdbg stats, runs, per-sequence list, path stats): runs a list of dicts with
    text_pos, seq, windows, unitig, pos, rev, joined in text order; the per-sequence list of dicts
    with first_run, windows, located, runs, chains, longest_chain.  graph: cdbg_model.cdbg's answer
    for the table and the range, when it is at hand"""
    if graph is not None:
        units, edges, cst = graph
    elif table:
        units, edges, cst = cm.cdbg(table, min_count, max_count)
    else:
        units, edges, cst = [], [], None
    where = places(units, k)
    have = set(edges)
    up = text.upper()
    runs, per = [], []
    for i in range(len(offsets) - 1):
        a, e = offsets[i], offsets[i + 1]
        rec = {"first_run": len(runs), "windows": 0, "located": 0, "runs": 0, "chains": 0, "longest_chain": 0}
        prev = None  # the place of the window at p - 1, None: not located or no window
        chain = 0
        for p in range(a, e - k + 1):
            w = up[p:p + k]
            pl = None
            if set(w) <= BASES:
                rec["windows"] += 1
                pl = locate(units, where, w)
            if pl is not None:
                rec["located"] += 1
                u, rev, q = pl
                n, circ = units[u][1], units[u][3]
                cont = prev is not None and prev[0] == u and prev[1] == rev and (
                    q == prev[2] + 1 or (circ and prev[2] == n - 1 and q == 0))
                if cont:
                    runs[-1]["windows"] += 1
                else:
                    runs.append({"text_pos": p, "seq": i, "windows": 1, "unitig": u, "pos": q, "rev": rev,
                                 "joined": int(prev is not None)})
                    rec["runs"] += 1
                if prev is None:
                    rec["chains"] += 1
                    chain = 0
                chain += 1
                rec["longest_chain"] = max(rec["longest_chain"], chain)
            prev = pl
        per.append(rec)
    # the properties include/kc_api.h states
    for j, r in enumerate(runs):
        n, circ = units[r["unitig"]][1], units[r["unitig"]][3]
        assert r["pos"] < n
        assert circ or r["pos"] + r["windows"] <= n
        if r["joined"]:
            b = runs[j - 1]
            assert b["seq"] == r["seq"] and b["text_pos"] + b["windows"] == r["text_pos"]
            assert r["pos"] == 0, "a joined run starts at q = 0"
            nb = units[b["unitig"]][1]
            assert (b["pos"] + b["windows"] - 1) % nb == nb - 1 and (units[b["unitig"]][3] or b["pos"] + b["windows"] == nb), \
                "the run before a joined run ends at the last k-mer of its oriented unitig"
            assert not circ and not units[b["unitig"]][3], "no run on a circular unitig is joined or followed by a joined run"
            assert (b["unitig"], b["rev"], r["unitig"], r["rev"]) in have, (b, r)
    # along a chain the text equals the walk's string
    j = 0
    while j < len(runs):
        walk = spelled(units[runs[j]["unitig"]], k, runs[j]["rev"], runs[j]["pos"], runs[j]["windows"])
        start, j = runs[j]["text_pos"], j + 1
        while j < len(runs) and runs[j]["joined"]:
            walk += spelled(units[runs[j]["unitig"]], k, runs[j]["rev"], runs[j]["pos"], runs[j]["windows"])[k - 1:]
            j += 1
        assert up[start:start + len(walk)] == walk, (start, walk)
    for rec in per:
        assert rec["located"] <= rec["windows"] and rec["chains"] <= rec["runs"] <= rec["located"]
    st = {"seqs": len(per), "windows": sum(r["windows"] for r in per), "located": sum(r["located"] for r in per),
          "runs": len(runs), "chains": sum(r["chains"] for r in per),
          "threaded": sum(1 for r in per if r["windows"] > 0 and r["longest_chain"] == r["windows"])}
    return units, edges, cst, runs, per, st


def count(seqs, k):
    """{canonical k-mer: occurrences} of sequences, breaks as the text's"""
    table = {}
    for s in seqs:
        s = s.upper()
        for p in range(len(s) - k + 1):
            w = s[p:p + k]
            if set(w) <= BASES:
                c = m.canon(w)
                table[c] = table.get(c, 0) + 1
    return table


def normalised_runs(units, runs):
    """[(text_pos, seq, windows, normal of the unitig, rev in the normal form, joined)] -- and for an
    open unitig q too: a unitig is named by unitig_model.normal and the strand bit is xored with "the
    string is not its normal form" (a palindrome never), so that the device's list and the model's
    compare whatever strand and start the unitigs were written from.  A circular unitig's q and
    strand depend on where it was cut and are left out; the spelling checks cover them."""
    import unitig_model as um
    out = []
    for r in runs:
        s, n, _, circ = units[r["unitig"]]
        nm = um.normal(s, n, circ)
        if circ:
            out.append((r["text_pos"], r["seq"], r["windows"], nm, None, None, r["joined"]))
        else:
            flip = 0 if s == m.rc(s) else int(s != nm)
            out.append((r["text_pos"], r["seq"], r["windows"], nm, r["rev"] ^ flip, r["pos"], r["joined"]))
    return out
