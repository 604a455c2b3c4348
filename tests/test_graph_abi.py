"""CPU: the de Bruijn graph entry points exist at the ABI boundary (kc_neighbors*, kc_graph*), the
Python mirror of kc_graph_stats matches the C struct, the GRAPH_* flags are the header's and the
model's, and a call without a context is refused before any device is touched."""
import ctypes
import os
import re

from conftest import LIB, REPO
import graph_model
import kaarme_amd as ka

GRAPH_SYMBOLS = ("kc_neighbors_device", "kc_neighbors", "kc_graph_device", "kc_graph")
KC_ERR_ARG = -1


def _header():
    with open(os.path.join(REPO, "include", "kc_api.h")) as f:
        return f.read()


def test_library_exports_graph_symbols():
    lib = ctypes.CDLL(LIB)
    for name in GRAPH_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in ka.EXPORTS


def test_header_declares_graph_entry_points():
    text = _header()
    for name in GRAPH_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*kc_ctx\s*\*" % name, text), name
    assert re.search(r"\bkc_neighbors_device\s*\([^;]*const\s+uint64_t\s*\*\s*dev_keys[^;]*uint32_t\s*\*\s*dev_counts[^;]*"
                     r"void\s*\*\s*hip_stream\s*\)\s*;", text)
    assert re.search(r"\bkc_graph_device\s*\([^;]*uint32_t\s+min_count\s*,\s*uint32_t\s+max_count\s*,\s*uint64_t\s*\*\s*"
                     r"dev_records\s*,\s*uint64_t\s+capacity\s*,\s*uint64_t\s*\*\s*dev_n_records\s*,\s*kc_graph_stats\s*\*"
                     r"\s*dev_stats\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", text)
    assert re.search(r"\bkc_graph\s*\([^;]*uint64_t\s*\*\*\s*records\s*,\s*uint64_t\s*\*\s*n_records\s*,\s*"
                     r"kc_graph_stats\s*\*\s*stats\s*\)\s*;", text)
    assert re.search(r"\}\s*kc_graph_stats\s*;", text)


def test_struct_layout():
    assert ctypes.sizeof(ka.kc_graph_stats) == 80
    names = [n for n, _ in ka.kc_graph_stats._fields_]
    assert tuple(names[:5]) == graph_model.FIELDS and names[5:] == ["side_degree"]
    assert [getattr(ka.kc_graph_stats, n).offset for n in names] == [0, 8, 16, 24, 32, 40]
    assert ka.kc_graph_stats.side_degree.size == 40
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*kc_graph_stats\s*;", _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"uint64_t\s+([^;]+);", body) == ["nodes", "edge_ends", "link_ends", "isolated", "palindromes",
                                                         "side_degree[5]"]
    st = ka.kc_graph_stats(7, 10, 4, 1, 0, (ctypes.c_uint64 * 5)(2, 12, 0, 0, 0))
    assert st.as_dict() == {"nodes": 7, "edge_ends": 10, "link_ends": 4, "isolated": 1, "palindromes": 0,
                            "side_degree": [2, 12, 0, 0, 0], "open_unitigs": 5}


def test_flag_values_are_the_headers():
    text = _header()
    for name, v in (("LINK_R", 0x100), ("LINK_L", 0x200), ("NODE", 0x8000)):
        found = re.search(r"#define\s+KC_GRAPH_%s\s+(0x[0-9A-Fa-f]+)u?\b" % name, text)
        assert found and int(found.group(1), 16) == v, name
        assert getattr(ka, "GRAPH_" + name) == v == getattr(graph_model, name)
    assert re.search(r"#define\s+KC_GRAPH_EDGE_R\(y\)\s+\(1u\s*<<\s*\(y\)\)", text)
    assert re.search(r"#define\s+KC_GRAPH_EDGE_L\(y\)\s+\(1u\s*<<\s*\(4\s*\+\s*\(y\)\)\)", text)


def test_null_context_is_an_argument_error():
    lib = ka.load_library()
    st = ka.kc_graph_stats()
    assert lib.kc_neighbors(None, None, 0, 0, None) == KC_ERR_ARG
    assert lib.kc_neighbors_device(None, None, 0, 0, None, None) == KC_ERR_ARG
    assert lib.kc_graph(None, 1, 0, None, None, ctypes.byref(st)) == KC_ERR_ARG
    assert lib.kc_graph_device(None, 1, 0, None, 0, None, None, None) == KC_ERR_ARG
