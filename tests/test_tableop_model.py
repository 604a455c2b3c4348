"""CPU: the pure-Python model of the table algebra (tableop_model.py) on hand-written dicts: all
seven operations, the ranges' edges, T(c) of each operand's own mode, and accumulation."""
import pytest

import tableop_model as m

A = {"AAA": 5, "AAC": 1, "AAG": 7, "ACA": 2, "ACC": 9}
B = {"AAA": 3, "AAG": 7, "ACA": 6, "CCC": 4, "CCG": 1}

WANT = {
    m.OP_INTERSECT_MIN: {"AAA": 3, "AAG": 7, "ACA": 2},
    m.OP_INTERSECT_SUM: {"AAA": 8, "AAG": 14, "ACA": 8},
    m.OP_INTERSECT_LEFT: {"AAA": 5, "AAG": 7, "ACA": 2},
    m.OP_SUBTRACT: {"AAC": 1, "ACC": 9},
    m.OP_COUNTS_SUBTRACT: {"AAA": 2, "AAC": 1, "ACC": 9},  # AAG 7 - 7 and ACA 2 - 6 are dropped
    m.OP_UNION_SUM: {"AAA": 8, "AAC": 1, "AAG": 14, "ACA": 8, "ACC": 9, "CCC": 4, "CCG": 1},
    m.OP_UNION_MAX: {"AAA": 5, "AAC": 1, "AAG": 7, "ACA": 6, "ACC": 9, "CCC": 4, "CCG": 1},
}


@pytest.mark.parametrize("op", m.OPS)
def test_every_operation(op):
    out, st = m.table_op(A, B, op)
    assert out == WANT[op]
    assert st["a_keys"] == 5 and st["both"] == 3
    assert st["b_only"] == (2 if op in m.UNION_OPS else 0)
    assert st["out_keys"] == len(WANT[op]) and st["out_sum"] == sum(WANT[op].values())
    assert tuple(st) == m.FIELDS


def test_names_follow_the_op_values():
    assert m.OP_NAMES[m.OP_SUBTRACT] == "subtract" and m.OP_NAMES[m.OP_UNION_MAX] == "union-max"
    assert len(m.OP_NAMES) == len(m.OPS) == 7


def test_range_edges():
    # a_min = 2 drops AAC (1); a_min 0 means 1; a max of 0 is no upper bound; both edges inclusive
    out, st = m.table_op(A, B, m.OP_INTERSECT_LEFT, a_range=(2, 0))
    assert st["a_keys"] == 4 and out == {"AAA": 5, "AAG": 7, "ACA": 2}
    assert m.table_op(A, B, m.OP_SUBTRACT, a_range=(0, 0)) == m.table_op(A, B, m.OP_SUBTRACT, a_range=(1, 0))
    out, st = m.table_op(A, B, m.OP_SUBTRACT, a_range=(2, 7))
    assert st["a_keys"] == 3 and st["both"] == 3 and out == {}
    out, st = m.table_op(A, B, m.OP_SUBTRACT, a_range=(5, 5))
    assert st["a_keys"] == 1 and out == {}
    # b_max = 1: only CCG is in b, so every key of a is "not in b"
    out, st = m.table_op(A, B, m.OP_SUBTRACT, b_range=(1, 1))
    assert st["both"] == 0 and out == A
    out, st = m.table_op(A, B, m.OP_COUNTS_SUBTRACT, b_range=(1, 1))
    assert out == A  # cb = 0 for a key of b outside b's range
    # a key outside a's range but inside b's comes out of a UNION as op(0, cb)
    for op in m.UNION_OPS:
        out, st = m.table_op(A, B, op, a_range=(6, 0))
        assert st == {"a_keys": 2, "both": 1, "b_only": 4, "out_keys": 6, "out_sum": sum(out.values())}
        assert out["AAA"] == 3 and out["ACA"] == 6 and out["CCC"] == 4 and "AAC" not in out
        assert out["AAG"] == (14 if op == m.OP_UNION_SUM else 7) and out["ACC"] == 9


def test_ranges_are_on_each_operands_own_tc():
    a = {"x": 20000, "y": 65536 + 3, "z": 65536}
    # -m 2: T = 16383 for x, y, z; -m 0: T = 20000, 3, 0 (z wrapped to 0: in no range)
    assert [m.tc(c, 2) for c in a.values()] == [16383] * 3
    assert [m.tc(c, 0) for c in a.values()] == [20000, 3, 0]
    out, st = m.table_op(a, {}, m.OP_SUBTRACT, mode_a=2, a_range=(16383, 16383))
    assert st["a_keys"] == 3 and out == a  # the raw counts move
    out, st = m.table_op(a, {}, m.OP_SUBTRACT, mode_a=0, a_range=(1, 10))
    assert out == {"y": 65539}
    out, st = m.table_op(a, {}, m.OP_SUBTRACT, mode_a=0)
    assert st["a_keys"] == 2 and "z" not in out
    # raw counts: the subtraction happens before the destination saturates
    out, _ = m.table_op({"p": 20000}, {"p": 17000}, m.OP_COUNTS_SUBTRACT)
    assert m.read_back(out, 2) == {"p": 3000}
    out, _ = m.table_op({"p": 20000}, {"p": 17000}, m.OP_INTERSECT_SUM)
    assert out == {"p": 37000} and m.read_back(out, 2) == {"p": 16383} and m.read_back(out, 0) == {"p": 37000}


def test_same_table_and_empty_operands():
    for op in m.OPS:
        out, st = m.table_op(A, A, op)
        assert st["a_keys"] == st["both"] == 5 and st["b_only"] == 0
        if op in (m.OP_SUBTRACT, m.OP_COUNTS_SUBTRACT):
            assert out == {}
        elif op in (m.OP_INTERSECT_SUM, m.OP_UNION_SUM):
            assert out == {key: 2 * c for key, c in A.items()}
        else:
            assert out == A
        out, st = m.table_op({}, B, op)
        assert st["a_keys"] == 0 and out == (B if op in m.UNION_OPS else {})
        out, st = m.table_op(A, {}, op)
        assert out == ({} if op in (m.OP_INTERSECT_MIN, m.OP_INTERSECT_SUM, m.OP_INTERSECT_LEFT) else A)


def test_results_accumulate_and_compare():
    dst = {}
    m.add_into(dst, m.table_op(A, B, m.OP_INTERSECT_MIN)[0])
    m.add_into(dst, m.table_op(A, B, m.OP_SUBTRACT)[0])
    assert dst == {"AAA": 3, "AAG": 7, "ACA": 2, "AAC": 1, "ACC": 9}
    assert m.read_back(dst, 2, min_abundance=3) == {"AAA": 3, "AAG": 7, "ACC": 9}
    c = m.compare(A, B)
    assert c["jaccard"] == 3 / 7 and c["containment"] == 3 / 5 and c["b_only"] == 2
    assert m.compare({}, {})["jaccard"] == 0.0
