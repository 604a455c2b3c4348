"""CPU: the read-correction entry points exist at the ABI boundary (kc_correct*), the Python mirrors
of kc_correct_stat match the C struct, and a NULL context is refused."""
import ctypes
import os
import re

from conftest import LIB, REPO
import kaarme_amd as ka
import correct_model

CORRECT_SYMBOLS = ("kc_correct_device", "kc_correct")
KC_ERR_ARG = -1


class kc_correct_stat(ctypes.Structure):  # include/kc_api.h
    _fields_ = [("candidates", ctypes.c_uint32), ("corrected", ctypes.c_uint32), ("ambiguous", ctypes.c_uint32),
                ("dropped", ctypes.c_uint32)]


def test_library_exports_correct_symbols():
    lib = ctypes.CDLL(LIB)
    for name in CORRECT_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in ka.EXPORTS


def test_header_declares_correct_entry_points():
    with open(os.path.join(REPO, "include", "kc_api.h")) as f:
        text = f.read()
    for name in CORRECT_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*kc_ctx\s*\*" % name, text), name
    assert re.search(r"\}\s*kc_correct_stat\s*;", text)
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*kc_correct_stat\s*;", text).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"uint32_t\s+(\w+)\s*;", body) == list(correct_model.FIELDS)


def test_correct_stat_layout():
    assert ctypes.sizeof(kc_correct_stat) == 16 == ctypes.sizeof(ka.kc_correct_stat)
    assert ka.CORRECT_STAT_DTYPE.itemsize == 16
    names = tuple(n for n, _ in kc_correct_stat._fields_)
    assert ka.CORRECT_STAT_DTYPE.names == names == correct_model.FIELDS
    assert tuple(n for n, _ in ka.kc_correct_stat._fields_) == names
    for i, name in enumerate(names):
        assert getattr(kc_correct_stat, name).offset == 4 * i == getattr(ka.kc_correct_stat, name).offset
        assert ka.CORRECT_STAT_DTYPE.fields[name][1] == 4 * i
        assert ka.CORRECT_STAT_DTYPE.fields[name][0].itemsize == 4


def test_null_context_is_an_argument_error():
    lib = ka.load_library()
    text = b"ACGT" * 10
    out = ctypes.create_string_buffer(len(text))
    off = (ctypes.c_uint64 * 2)(0, len(text))
    assert lib.kc_correct(None, text, len(text), off, 1, 1, out, None) == KC_ERR_ARG
    assert lib.kc_correct_device(None, None, 0, None, 0, 1, None, None, None) == KC_ERR_ARG
    assert out.raw == b"\0" * len(text)
