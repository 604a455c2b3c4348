"""Pure-Python model of the table algebra (include/kc_api.h kc_table_op): two {k-mer: raw count}
dicts, the operands' modes, the operation and the two ranges in; the result {k-mer: raw count} and
the five statistics of kc_op_stats out.  The GPU tests compare the engine against it."""

OP_INTERSECT_MIN, OP_INTERSECT_SUM, OP_INTERSECT_LEFT, OP_SUBTRACT, OP_COUNTS_SUBTRACT, OP_UNION_SUM, OP_UNION_MAX = range(7)
OPS = tuple(range(7))
UNION_OPS = (OP_UNION_SUM, OP_UNION_MAX)
OP_NAMES = ("intersect-min", "intersect-sum", "intersect-left", "subtract", "counts-subtract", "union-sum",
            "union-max")
FIELDS = ("a_keys", "both", "b_only", "out_keys", "out_sum")


def tc(c, mode):
    """T(c) as kc_dump and kc_lookup report a raw count: c mod 65536 for -m 0, min(c, 16383) otherwise"""
    return c % 65536 if mode == 0 else min(c, 16383)


def in_range(c, mode, rng):
    """a key takes part when lo <= T(c) <= hi; lo 0 means 1, hi 0 means no upper bound"""
    lo, hi = rng
    t = tc(c, mode)
    return t >= (lo or 1) and (hi == 0 or t <= hi)


def apply(op, ca, cb):
    """the operation on raw counts, cb = 0 (or ca = 0) for a key the table does not hold; 0 = no record"""
    if op == OP_INTERSECT_MIN:
        return min(ca, cb) if ca and cb else 0
    if op == OP_INTERSECT_SUM:
        return ca + cb if ca and cb else 0
    if op == OP_INTERSECT_LEFT:
        return ca if ca and cb else 0
    if op == OP_SUBTRACT:
        return ca if not cb else 0
    if op == OP_COUNTS_SUBTRACT:
        return ca - cb if ca > cb else 0
    if op == OP_UNION_SUM:
        return ca + cb
    if op == OP_UNION_MAX:
        return max(ca, cb)
    raise ValueError(f"unknown op {op}")


def table_op(a, b, op, mode_a=2, mode_b=2, a_range=(1, 0), b_range=(1, 0)):
    """(result, stats): result = {key: raw count} of the records the operation yields"""
    ina = {key: c for key, c in a.items() if c and in_range(c, mode_a, a_range)}
    inb = {key: c for key, c in b.items() if c and in_range(c, mode_b, b_range)}
    out = {}
    for key, ca in ina.items():
        r = apply(op, ca, inb.get(key, 0))
        if r:
            out[key] = r
    b_only = 0
    if op in UNION_OPS:  # the only ones that sweep b
        for key, cb in inb.items():
            if key not in ina:
                b_only += 1
                out[key] = apply(op, 0, cb)
    stats = {"a_keys": len(ina), "both": sum(1 for key in ina if key in inb), "b_only": b_only,
             "out_keys": len(out), "out_sum": sum(out.values())}
    return out, stats


def add_into(dst, result):
    """results are ADDED into the destination's raw counts"""
    for key, c in result.items():
        dst[key] = dst.get(key, 0) + c
    return dst


def read_back(raw, mode, min_abundance=1):
    """what kc_dump of a table with these raw counts reports: {key: T(c)} for T(c) >= a"""
    return {key: tc(c, mode) for key, c in raw.items() if tc(c, mode) >= min_abundance}


def compare(a, b, mode_a=2, mode_b=2, a_range=(1, 0), b_range=(1, 0)):
    """table_compare: the statistics of UNION_SUM plus jaccard and containment (of a in b)"""
    _, st = table_op(a, b, OP_UNION_SUM, mode_a, mode_b, a_range, b_range)
    union = st["a_keys"] + st["b_only"]
    st["jaccard"] = st["both"] / union if union else 0.0
    st["containment"] = st["both"] / st["a_keys"] if st["a_keys"] else 0.0
    return st
