"""CPU: the sequence-query entry points exist at the ABI boundary (kc_text_counts*, kc_seq_stats*),
the Python mirror of kc_seq_stat matches the C struct, pack_sequences round-trips, and the
pure-Python model the GPU tests compare against (seq_model.py) agrees with a brute-force count."""
import ctypes
import os
import re

import numpy as np

from conftest import LIB, REPO
import kaarme_amd as ka
import seq_model

SEQ_SYMBOLS = ("kc_text_counts_device", "kc_text_counts", "kc_seq_stats_device", "kc_seq_stats")


class kc_seq_stat(ctypes.Structure):  # include/kc_api.h
    _fields_ = [("windows", ctypes.c_uint32), ("present", ctypes.c_uint32), ("solid", ctypes.c_uint32),
                ("min", ctypes.c_uint32), ("median", ctypes.c_uint32), ("max", ctypes.c_uint32),
                ("sum", ctypes.c_uint64)]


def test_library_exports_seq_symbols():
    lib = ctypes.CDLL(LIB)
    for name in SEQ_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in ka.EXPORTS


def test_header_declares_seq_entry_points():
    with open(os.path.join(REPO, "include", "kc_api.h")) as f:
        text = f.read()
    for name in SEQ_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*kc_ctx\s*\*" % name, text), name
    assert re.search(r"#define\s+KC_NO_KMER\s+0xFFFFFFFFu\b", text)
    assert ka.NO_KMER == 0xFFFFFFFF == seq_model.NO_KMER
    assert re.search(r"\}\s*kc_seq_stat\s*;", text)


def test_seq_stat_layout():
    assert ctypes.sizeof(kc_seq_stat) == 32
    assert ka.SEQ_STAT_DTYPE.itemsize == 32
    assert ka.SEQ_STAT_DTYPE.names == tuple(n for n, _ in kc_seq_stat._fields_) == seq_model.FIELDS
    for name, _ in kc_seq_stat._fields_:
        assert ka.SEQ_STAT_DTYPE.fields[name][1] == getattr(kc_seq_stat, name).offset, name
        assert ka.SEQ_STAT_DTYPE.fields[name][0].itemsize == getattr(kc_seq_stat, name).size, name


def test_pack_sequences_round_trips():
    seqs = ["ACGT", "", b"NNacgt", "T", ""]
    text, off = ka.pack_sequences(seqs)
    assert off.dtype == np.uint64 and len(off) == len(seqs) + 1 and off[0] == 0 and off[-1] == len(text)
    back = [text[int(off[i]):int(off[i + 1]) - 1] for i in range(len(seqs))]
    assert back == [s.encode() if isinstance(s, str) else s for s in seqs]
    assert all(text[int(o) - 1:int(o)] == b"\n" for o in off[1:])
    text, off = ka.pack_sequences([])
    assert text == b"" and off.tolist() == [0]


def _brute(text, k, d):
    """counts by the definition, no rolling state"""
    out = []
    for p in range(len(text)):
        w = text[p:p + k]
        if len(w) < k or any(c not in b"ACGTacgt" for c in w):
            out.append(seq_model.NO_KMER)
            continue
        w = w.upper()
        rc = bytes({65: 84, 67: 71, 71: 67, 84: 65}[c] for c in reversed(w))
        out.append(d.get(min(w, rc), 0))
    return out


def test_seq_model_against_brute_force():
    k = 3
    text = b"ACGTTnACG\nAAATTTgca>ACCGGT"
    # counts of the canonical 3-mers of a made-up table
    d = {b"ACG": 5, b"AAC": 2, b"AAA": 7, b"AAT": 1, b"GCA": 9, b"ACC": 3, b"CCG": 4}
    assert all(seq_model.canonical(s) == s for s in d)
    want = _brute(text, k, d)
    assert seq_model.text_counts(text, k, d) == want
    assert want[0] == 5 and want[1] == 5 and want[2] == 2  # ACG, CGT = rc ACG, GTT = rc AAC
    assert want[4] == want[5] == seq_model.NO_KMER          # windows over the 'n'
    assert want[16] == 9 and want[-2:] == [seq_model.NO_KMER] * 2
    # sequences by offsets: windows stay inside, also with no break byte between two of them
    off = [0, 5, 5, 9, 10, 19, 26]
    st = seq_model.seq_stats(text, off, k, d, solid_min=5)
    for i, s in enumerate(st):
        vals = [v for v in _brute(text[off[i]:off[i + 1]], k, d) if v != seq_model.NO_KMER]
        assert s["windows"] == len(vals)
        if vals:
            assert s["sum"] == sum(vals) and s["min"] == min(vals) and s["max"] == max(vals)
            assert s["median"] == sorted(vals)[(len(vals) - 1) // 2]
            assert s["present"] == sum(v > 0 for v in vals) and s["solid"] == sum(v >= 5 for v in vals)
    assert st[0] == {"windows": 3, "present": 3, "solid": 2, "min": 2, "median": 5, "max": 5, "sum": 12}
    assert st[1] == dict.fromkeys(seq_model.FIELDS, 0)
    assert st[2]["windows"] == 1  # "nACG": the joint with "ACGTT" adds no window
    assert seq_model.stats_of([4, 1, 3, 2], 2)["median"] == 2  # the lower median of an even number
    assert seq_model.revcomp(b"AACG") == b"CGTT"
