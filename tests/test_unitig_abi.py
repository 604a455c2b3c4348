"""CPU: the unitig entry points exist at the ABI boundary (kc_unitigs*), the Python mirrors of
kc_unitig and kc_unitig_stats match the C structs, the flag is the header's, and a call without a
context is refused before any device is touched."""
import ctypes
import os
import re

import numpy as np

from conftest import LIB, REPO
import kaarme_amd as ka

UNITIG_SYMBOLS = ("kc_unitigs_device", "kc_unitigs")
KC_ERR_ARG = -1


def _header():
    with open(os.path.join(REPO, "include", "kc_api.h")) as f:
        return f.read()


def _fields(name):
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [n.strip() for decl in re.findall(r"uint64_t\s+([^;]+);", body) for n in decl.split(",")]


def test_library_exports_unitig_symbols():
    lib = ctypes.CDLL(LIB)
    for name in UNITIG_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in ka.EXPORTS


def test_header_declares_unitig_entry_points():
    text = _header()
    for name in UNITIG_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*kc_ctx\s*\*" % name, text), name
    assert re.search(r"\bkc_unitigs_device\s*\([^;]*uint32_t\s+min_count\s*,\s*uint32_t\s+max_count\s*,\s*kc_unitig\s*\*\s*"
                     r"dev_unitigs\s*,\s*uint64_t\s+cap_unitigs\s*,\s*uint8_t\s*\*\s*dev_bases\s*,\s*uint64_t\s+cap_bases\s*,"
                     r"\s*kc_unitig_stats\s*\*\s*dev_stats\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", text)
    assert re.search(r"\bkc_unitigs\s*\([^;]*kc_unitig\s*\*\*\s*unitigs\s*,\s*uint8_t\s*\*\*\s*bases\s*,\s*"
                     r"kc_unitig_stats\s*\*\s*stats\s*\)\s*;", text)
    assert re.search(r"\}\s*kc_unitig\s*;", text) and re.search(r"\}\s*kc_unitig_stats\s*;", text)


def test_struct_layout():
    assert ctypes.sizeof(ka.kc_unitig) == 32 and ctypes.sizeof(ka.kc_unitig_stats) == 40
    for cls, name in ((ka.kc_unitig, "kc_unitig"), (ka.kc_unitig_stats, "kc_unitig_stats")):
        names = [n for n, _ in cls._fields_]
        assert names == _fields(name), name
        assert [getattr(cls, n).offset for n in names] == [8 * i for i in range(len(names))]
    assert _fields("kc_unitig") == ["offset", "n_nodes", "count_sum", "flags"]
    assert _fields("kc_unitig_stats") == ["unitigs", "circular", "nodes", "bases", "max_nodes"]
    assert re.search(r"typedef\s+struct\s*\{\s*/\*\s*32 bytes\s*\*/[^}]*\}\s*kc_unitig\s*;", _header())
    assert re.search(r"typedef\s+struct\s*\{\s*/\*\s*40 bytes\s*\*/[^}]*\}\s*kc_unitig_stats\s*;", _header())
    assert ka.kc_unitig(5, 3, 9, 1).as_dict() == {"offset": 5, "n_nodes": 3, "count_sum": 9, "flags": 1}
    assert ka.kc_unitig_stats(2, 1, 7, 13, 5).as_dict() == {"unitigs": 2, "circular": 1, "nodes": 7, "bases": 13,
                                                            "max_nodes": 5}


def test_flag_value_is_the_headers():
    found = re.search(r"#define\s+KC_UNITIG_CIRCULAR\s+(\d+)u?\b", _header())
    assert found and int(found.group(1)) == ka.UNITIG_CIRCULAR == 1


def test_unitig_strings_cuts_the_bases():
    bases = np.frombuffer(b"ACGTACGGTT", dtype=np.uint8)
    records = np.array([[4, 4, 9, 0], [0, 2, 3, 1]], dtype=np.uint64)
    assert ka.unitig_strings(records, bases, 3) == ["ACGGTT", "ACGT"]
    assert ka.unitig_strings(np.zeros((0, 4), dtype=np.uint64), bases, 3) == []


def test_null_context_is_an_argument_error():
    lib = ka.load_library()
    st = ka.kc_unitig_stats()
    assert lib.kc_unitigs(None, 1, 0, None, None, ctypes.byref(st)) == KC_ERR_ARG
    assert lib.kc_unitigs_device(None, 1, 0, None, 0, None, 0, None, None) == KC_ERR_ARG
