"""CPU: the read-path entry points exist at the ABI boundary (kc_read_paths*), the Python mirrors of
kc_path_run, kc_path_seq and kc_path_stats match the C structs field by field, the flags are the
header's, and a call without a context is refused before any device is touched."""
import ctypes
import os
import re

import numpy as np

from conftest import LIB, REPO
import kaarme_amd as ka

PATH_SYMBOLS = ("kc_read_paths_device", "kc_read_paths")
KC_ERR_ARG = -1
RUN_FIELDS = [("text_pos", 8), ("seq", 4), ("windows", 4), ("unitig", 4), ("pos", 4), ("flags", 4), ("reserved", 4)]
SEQ_FIELDS = [("first_run", 8), ("windows", 4), ("located", 4), ("runs", 4), ("chains", 4), ("longest_chain", 4),
              ("reserved", 4)]
STAT_FIELDS = ["seqs", "windows", "located", "runs", "chains", "threaded"]


def _header():
    with open(os.path.join(REPO, "include", "kc_api.h")) as f:
        return f.read()


def _fields(name):
    """[(field, bytes)] of the struct in the header, in order (arrays: the whole array's bytes)"""
    body = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*%s\s*;" % name, _header()).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for d in (d.strip() for d in body.split(";")):
        if not d:
            continue
        ctype, names = d.split(None, 1)
        size = {"uint64_t": 8, "uint32_t": 4}[ctype]
        for n in names.split(","):
            arr = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", n)
            out.append((arr.group(1), size * int(arr.group(2) or 1)))
    return out


def test_library_exports_path_symbols():
    lib = ctypes.CDLL(LIB)
    for name in PATH_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in ka.EXPORTS


def test_header_declares_path_entry_points():
    text = re.sub(r"\s+", " ", _header())
    assert ("int kc_read_paths_device(kc_ctx* ctx, uint32_t min_count, uint32_t max_count, kc_unitig* dev_unitigs, "
            "uint64_t cap_unitigs, uint8_t* dev_bases, uint64_t cap_bases, kc_unitig_edge* dev_edges, uint64_t cap_edges, "
            "kc_cdbg_stats* dev_cdbg_stats, const uint8_t* dev_text, uint64_t n_bytes, const uint64_t* offsets, "
            "uint64_t n_seqs, kc_path_run* dev_runs, uint64_t cap_runs, kc_path_seq* dev_seq, "
            "kc_path_stats* dev_path_stats, void* hip_stream);") in text
    assert ("int kc_read_paths(kc_ctx* ctx, uint32_t min_count, uint32_t max_count, kc_unitig** unitigs, uint8_t** bases, "
            "kc_unitig_edge** edges, kc_cdbg_stats* cdbg_stats, const uint8_t* text, uint64_t n_bytes, "
            "const uint64_t* offsets, uint64_t n_seqs, kc_path_run** runs, kc_path_seq** seq, "
            "kc_path_stats* path_stats);") in text


def test_struct_mirrors_match_the_header():
    assert ctypes.sizeof(ka.kc_path_run) == 32 and ctypes.sizeof(ka.kc_path_seq) == 32 and ctypes.sizeof(ka.kc_path_stats) == 64
    assert _fields("kc_path_run") == RUN_FIELDS and _fields("kc_path_seq") == SEQ_FIELDS
    assert _fields("kc_path_stats") == [(n, 8) for n in STAT_FIELDS] + [("reserved", 16)]
    for cls, fields, dtype in ((ka.kc_path_run, RUN_FIELDS, ka.RUN_DTYPE), (ka.kc_path_seq, SEQ_FIELDS, ka.PATH_SEQ_DTYPE)):
        assert [n for n, _ in cls._fields_] == [n for n, _ in fields]
        at = 0
        for n, size in fields:
            assert getattr(cls, n).offset == at and getattr(cls, n).size == size, n
            # the numpy view is the same 32 bytes
            assert dtype.fields[n] == (np.dtype("<u%d" % size), at), n
            at += size
        assert at == 32 == dtype.itemsize and list(dtype.names) == [n for n, _ in fields]
    assert [n for n, _ in ka.kc_path_stats._fields_] == STAT_FIELDS + ["reserved"]
    assert [getattr(ka.kc_path_stats, n).offset for n in STAT_FIELDS] == [8 * i for i in range(6)]
    assert ka.kc_path_stats.reserved.offset == 48 and ka.kc_path_stats.reserved.size == 16
    for name, size in (("kc_path_run", 32), ("kc_path_seq", 32), ("kc_path_stats", 64)):
        assert re.search(r"typedef\s+struct\s*\{\s*/\*\s*%d bytes[^*]*\*/[^}]*\}\s*%s\s*;" % (size, name), _header()), name
    assert ka.kc_path_stats(3, 90, 80, 5, 4, 2).as_dict() == {
        "seqs": 3, "windows": 90, "located": 80, "runs": 5, "chains": 4, "threaded": 2}


def test_flag_values_are_the_headers():
    for name, value in (("KC_RUN_REV", ka.RUN_REV), ("KC_RUN_JOINED", ka.RUN_JOINED)):
        found = re.search(r"#define\s+%s\s+(\d+)u?\b" % name, _header())
        assert found and int(found.group(1)) == value, name
    found = re.search(r"#define\s+KC_NO_UNITIG\s+(0x[0-9A-Fa-f]+)u?\b", _header())
    assert found and int(found.group(1), 16) == ka.NO_UNITIG == 0xFFFFFFFF
    assert (ka.RUN_REV, ka.RUN_JOINED) == (1, 2)


def test_null_context_is_an_argument_error():
    lib = ka.load_library()
    st = ka.kc_path_stats()
    off = np.zeros(2, dtype=np.uint64)
    assert lib.kc_read_paths(None, 1, 0, None, None, None, None, None, 0, off.ctypes.data, 1, None, None,
                             ctypes.byref(st)) == KC_ERR_ARG
    assert lib.kc_read_paths_device(None, 1, 0, None, 0, None, 0, None, 0, None, None, 0, off.ctypes.data, 1, None, 0,
                                    None, None, None) == KC_ERR_ARG


def test_gaf_lines_of_written_out_runs():
    """the GAF bookkeeping on runs written by hand: a chain over two segments, a second chain of the
    same read on the reverse strand, and a run 2.4 times round a circle of 5 nodes"""
    k = 5
    names, seqs = ["r0", "r1"], ["A" * 30, "C" * 20]
    records = np.array([[0, 10, 0, 0], [14, 4, 0, 0], [22, 5, 0, 1]], dtype=np.uint64)
    runs = np.zeros(4, dtype=ka.RUN_DTYPE)
    runs[0] = (2, 0, 3, 0, 7, 0, 0)                         # windows 2..4 on segment 0 from q = 7 to its end
    runs[1] = (5, 0, 4, 1, 0, ka.RUN_REV | ka.RUN_JOINED, 0)  # joined: all of segment 1, reversed
    runs[2] = (20, 0, 2, 1, 1, 0, 0)                        # a chain of its own
    runs[3] = (31 + 1, 1, 12, 2, 3, ka.RUN_REV, 0)           # 12 windows from q = 3 round 5 nodes: three visits
    assert ka.gaf_lines(names, seqs, records, runs, k) == [
        "r0\t30\t2\t13\t+\t>0<1\t18\t7\t18\t11\t11\t255\tcg:Z:11=",
        "r0\t30\t20\t26\t+\t>1\t8\t1\t7\t6\t6\t255\tcg:Z:6=",
        "r1\t20\t1\t17\t+\t<2<2<2\t19\t3\t19\t16\t16\t255\tcg:Z:16=",
    ]
