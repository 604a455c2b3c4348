"""CPU: the table-algebra entry points exist at the ABI boundary (kc_table_op*), the Python mirrors
of kc_op_desc / kc_op_stats match the C structs, the OP_* values are the header's, and a call with
no operands is refused before any device is touched."""
import ctypes
import os
import re

from conftest import LIB, REPO
import kaarme_amd as ka
import tableop_model

OP_SYMBOLS = ("kc_table_op_device", "kc_table_op")
KC_ERR_ARG = -1


def _header():
    with open(os.path.join(REPO, "include", "kc_api.h")) as f:
        return f.read()


def test_library_exports_table_op_symbols():
    lib = ctypes.CDLL(LIB)
    for name in OP_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in ka.EXPORTS


def test_header_declares_table_op_entry_points():
    text = _header()
    for name in OP_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*kc_ctx\s*\*\s*dst\s*,\s*kc_ctx\s*\*\s*a\s*,\s*kc_ctx\s*\*\s*b\b" % name, text), name
    assert re.search(r"\}\s*kc_op_desc\s*;", text) and re.search(r"\}\s*kc_op_stats\s*;", text)


def test_struct_layouts():
    assert ctypes.sizeof(ka.kc_op_desc) == 24
    assert ctypes.sizeof(ka.kc_op_stats) == 40
    assert [n for n, _ in ka.kc_op_desc._fields_] == ["op", "a_min", "a_max", "b_min", "b_max", "reserved"]
    assert [getattr(ka.kc_op_desc, n).offset for n, _ in ka.kc_op_desc._fields_] == [0, 4, 8, 12, 16, 20]
    assert tuple(n for n, _ in ka.kc_op_stats._fields_) == tableop_model.FIELDS
    assert [getattr(ka.kc_op_stats, n).offset for n in tableop_model.FIELDS] == [0, 8, 16, 24, 32]


def test_op_values_are_the_headers():
    text = _header()
    want = {"INTERSECT_MIN": 0, "INTERSECT_SUM": 1, "INTERSECT_LEFT": 2, "SUBTRACT": 3, "COUNTS_SUBTRACT": 4,
            "UNION_SUM": 5, "UNION_MAX": 6}
    for name, v in want.items():
        assert re.search(r"#define\s+KC_OP_%s\s+%d\b" % (name, v), text), name
        assert getattr(ka, "OP_" + name) == v == getattr(tableop_model, "OP_" + name)
    assert ka.OP_NAMES == {n: i for i, n in enumerate(tableop_model.OP_NAMES)}


def test_null_operands_are_an_argument_error():
    lib = ka.load_library()
    assert lib.kc_table_op(None, None, None, None, None) == KC_ERR_ARG
    assert lib.kc_table_op_device(None, None, None, None, None, None) == KC_ERR_ARG
    d = ka.kc_op_desc(ka.OP_UNION_SUM, 1, 0, 1, 0, 0)
    assert lib.kc_table_op(None, None, None, ctypes.byref(d), None) == KC_ERR_ARG
