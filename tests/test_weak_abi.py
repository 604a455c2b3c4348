"""CPU: the weak-link entry points exist at the ABI boundary (kc_cut_weak*), the Python mirrors of
kc_weak_desc and kc_weak_stats match the C structs field by field, and a call without a source or a
descriptor is refused before any device is touched."""
import ctypes
import os
import re

from conftest import LIB, REPO
import kaarme_amd as ka

WEAK_SYMBOLS = ("kc_cut_weak_device", "kc_cut_weak")
KC_ERR_ARG = -1
DESC_FIELDS = ["min_count", "max_count", "max_nodes", "ratio_permille", "max_mean", "reserved"]
STAT_FIELDS = ["unitigs", "nodes", "interior", "weak", "cut", "cut_nodes", "out_keys", "out_sum"]


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


def test_library_exports_weak_symbols():
    lib = ctypes.CDLL(LIB)
    for name in WEAK_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in ka.EXPORTS


def test_header_declares_weak_entry_points():
    text = _header()
    assert re.search(r"\bint\s+kc_cut_weak_device\s*\(\s*kc_ctx\s*\*\s*dst\s*,\s*kc_ctx\s*\*\s*src\s*,\s*const\s+kc_weak_desc\s*\*"
                     r"\s*d\s*,\s*kc_weak_stats\s*\*\s*dev_stats\s*,\s*void\s*\*\s*hip_stream\s*\)\s*;", text)
    assert re.search(r"\bint\s+kc_cut_weak\s*\(\s*kc_ctx\s*\*\s*dst\s*,\s*kc_ctx\s*\*\s*src\s*,\s*const\s+kc_weak_desc\s*\*\s*d\s*,"
                     r"\s*kc_weak_stats\s*\*\s*stats\s*\)\s*;", text)


def test_struct_mirrors_match_the_header():
    assert ctypes.sizeof(ka.kc_weak_desc) == 24 and ctypes.sizeof(ka.kc_weak_stats) == 64
    assert _fields("kc_weak_desc", "uint32_t") == DESC_FIELDS
    assert _fields("kc_weak_stats", "uint64_t") == STAT_FIELDS
    for cls, names, size in ((ka.kc_weak_desc, DESC_FIELDS, 4), (ka.kc_weak_stats, STAT_FIELDS, 8)):
        assert [n for n, _ in cls._fields_] == names
        assert [getattr(cls, n).offset for n in names] == [size * i for i in range(len(names))]
        assert all(getattr(cls, n).size == size for n in names)
    assert re.search(r"typedef\s+struct\s*\{\s*/\*\s*24 bytes\s*\*/[^}]*\}\s*kc_weak_desc\s*;", _header())
    assert re.search(r"typedef\s+struct\s*\{\s*/\*\s*64 bytes\s*\*/[^}]*\}\s*kc_weak_stats\s*;", _header())
    assert ka.kc_weak_desc(2, 50, 30, 200, 7, 0).as_dict() == dict(zip(DESC_FIELDS, (2, 50, 30, 200, 7, 0)))
    assert ka.kc_weak_stats(9, 8, 7, 6, 5, 4, 3, 2).as_dict() == dict(zip(STAT_FIELDS, (9, 8, 7, 6, 5, 4, 3, 2)))


def test_null_source_or_descriptor_is_an_argument_error():
    lib = ka.load_library()
    d, st = ka.kc_weak_desc(1, 0, 30, 200, 0, 0), ka.kc_weak_stats()
    assert lib.kc_cut_weak(None, None, ctypes.byref(d), ctypes.byref(st)) == KC_ERR_ARG
    assert lib.kc_cut_weak(None, None, None, None) == KC_ERR_ARG
    assert lib.kc_cut_weak_device(None, None, ctypes.byref(d), None, None) == KC_ERR_ARG
    assert lib.kc_cut_weak_device(None, None, None, None, None) == KC_ERR_ARG


def test_header_states_the_scratch_and_python_has_the_calls():
    section = _header().split("Weak-link removal:")[1].split("kc_weak_desc;")[0]
    assert "scratch = 5 * table_slots + 141 * ids bytes" in section
    for name in ("cut_weak_device", "cut_weak"):
        assert callable(getattr(ka.KmerCounter, name))
    assert callable(ka.weak_stats) and callable(ka.weak_rounds)
