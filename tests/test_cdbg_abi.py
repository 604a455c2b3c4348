"""CPU: the compacted-graph entry points exist at the ABI boundary (kc_unitig_graph*), the Python
mirrors of kc_unitig_edge and kc_cdbg_stats match the C structs field by field, the flags are the
header's, and a call without a context is refused before any device is touched."""
import ctypes
import os
import re

import numpy as np

from conftest import LIB, REPO
import kaarme_amd as ka

CDBG_SYMBOLS = ("kc_unitig_graph_device", "kc_unitig_graph")
KC_ERR_ARG = -1
EDGE_FIELDS = ["from", "to", "flags", "reserved"]
STAT_FIELDS = ["unitigs", "circular", "nodes", "bases", "max_nodes", "edges", "dead_ends", "reserved"]


def _header():
    with open(os.path.join(REPO, "include", "kc_api.h")) as f:
        return f.read()


def _fields(name, ctype):
    """the names of the struct's fields, in order; all are of `ctype`"""
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert all(d.startswith(ctype + " ") for d in decls), decls
    return [n.strip() for d in decls for n in d[len(ctype):].split(",")]


def test_library_exports_cdbg_symbols():
    lib = ctypes.CDLL(LIB)
    for name in CDBG_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in ka.EXPORTS


def test_header_declares_cdbg_entry_points():
    text = _header()
    assert re.search(r"\bint\s+kc_unitig_graph_device\s*\(\s*kc_ctx\s*\*\s*ctx\s*,\s*uint32_t\s+min_count\s*,\s*uint32_t\s+"
                     r"max_count\s*,\s*kc_unitig\s*\*\s*dev_unitigs\s*,\s*uint64_t\s+cap_unitigs\s*,\s*uint8_t\s*\*\s*"
                     r"dev_bases\s*,\s*uint64_t\s+cap_bases\s*,\s*kc_unitig_edge\s*\*\s*dev_edges\s*,\s*uint64_t\s+cap_edges"
                     r"\s*,\s*kc_cdbg_stats\s*\*\s*dev_stats\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", text)
    assert re.search(r"\bint\s+kc_unitig_graph\s*\(\s*kc_ctx\s*\*\s*ctx\s*,\s*uint32_t\s+min_count\s*,\s*uint32_t\s+max_count"
                     r"\s*,\s*kc_unitig\s*\*\*\s*unitigs\s*,\s*uint8_t\s*\*\*\s*bases\s*,\s*kc_unitig_edge\s*\*\*\s*edges\s*,"
                     r"\s*kc_cdbg_stats\s*\*\s*stats\s*\)\s*;", text)


def test_struct_mirrors_match_the_header():
    assert ctypes.sizeof(ka.kc_unitig_edge) == 16 and ctypes.sizeof(ka.kc_cdbg_stats) == 64
    assert _fields("kc_unitig_edge", "uint32_t") == EDGE_FIELDS
    assert _fields("kc_cdbg_stats", "uint64_t") == STAT_FIELDS
    for cls, names, size in ((ka.kc_unitig_edge, EDGE_FIELDS, 4), (ka.kc_cdbg_stats, STAT_FIELDS, 8)):
        assert [n for n, _ in cls._fields_] == names
        assert [getattr(cls, n).offset for n in names] == [size * i for i in range(len(names))]
        assert all(getattr(cls, n).size == size for n in names)
    assert re.search(r"typedef\s+struct\s*\{\s*/\*\s*16 bytes\s*\*/[^}]*\}\s*kc_unitig_edge\s*;", _header())
    assert re.search(r"typedef\s+struct\s*\{\s*/\*\s*64 bytes\s*\*/[^}]*\}\s*kc_cdbg_stats\s*;", _header())
    # the numpy view of the edges is the same 16 bytes
    assert ka.EDGE_DTYPE.itemsize == 16 and list(ka.EDGE_DTYPE.names) == EDGE_FIELDS
    assert [ka.EDGE_DTYPE.fields[n][1] for n in EDGE_FIELDS] == [0, 4, 8, 12]
    assert all(ka.EDGE_DTYPE.fields[n][0] == np.dtype("<u4") for n in EDGE_FIELDS)
    assert ka.kc_unitig_edge(5, 3, 2, 0).as_dict() == {"from": 5, "to": 3, "flags": 2, "reserved": 0}
    assert ka.kc_cdbg_stats(2, 1, 7, 13, 5, 4, 3, 0).as_dict() == {
        "unitigs": 2, "circular": 1, "nodes": 7, "bases": 13, "max_nodes": 5, "edges": 4, "dead_ends": 3}


def test_flag_values_are_the_headers():
    for name, value in (("KC_EDGE_FROM_REV", ka.EDGE_FROM_REV), ("KC_EDGE_TO_REV", ka.EDGE_TO_REV)):
        found = re.search(r"#define\s+%s\s+(\d+)u?\b" % name, _header())
        assert found and int(found.group(1)) == value, name
    assert (ka.EDGE_FROM_REV, ka.EDGE_TO_REV) == (1, 2)


def test_null_context_is_an_argument_error():
    lib = ka.load_library()
    st = ka.kc_cdbg_stats()
    assert lib.kc_unitig_graph(None, 1, 0, None, None, None, ctypes.byref(st)) == KC_ERR_ARG
    assert lib.kc_unitig_graph_device(None, 1, 0, None, 0, None, 0, None, 0, None, None) == KC_ERR_ARG
