"""kaarme_amd -- Python host mirror of the MI355X canonical k-mer counting engine.

Thin ctypes binding over ``lib/libkc.so`` (C ABI in ``include/kc_api.h``).  It mirrors
the reference's operator interface for the hot path: the ``parse_input_*`` functors
(``include/parallel_parser.hpp``) become :func:`count_file` / :class:`KmerCounter`,
``hash_kmers(chunk, format)`` becomes :meth:`KmerCounter.count_chunk`, the Bloom pass
``bloom_filter_kmers`` becomes :meth:`KmerCounter.bloom_chunk`, and the writers
(``write_kmers_on_disk_separately_even_faster`` / ``write_kmers``) become
:meth:`KmerCounter.write`.

There is no CPU fallback: if ``libkc.so`` is missing or no HIP device is usable, the
calls raise.  PyTorch is optional and only used by ``bench.py`` for device buffers,
streams and ``torch.distributed``.
"""
from __future__ import annotations

import ctypes
import dataclasses
import os
from dataclasses import dataclass
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# KC_LIB overrides the library (A/B runs of two builds); default: the in-tree build
LIB_PATH = os.environ.get("KC_LIB") or os.path.join(PKG_ROOT, "lib", "libkc.so")
CLI_PATH = os.path.join(PKG_ROOT, "bin", "kaarme")
GEN_PATH = os.path.join(PKG_ROOT, "bin", "kc_gen")

KC_OK = 0
ERRORS = {
    -1: "KC_ERR_ARG",
    -2: "KC_ERR_HIP",
    -3: "KC_ERR_TABLE_FULL",
    -4: "KC_ERR_STATE",
    -5: "KC_ERR_IO",
    -6: "KC_ERR_NOMEM",
    -7: "KC_ERR_UNSUPPORTED",
}
FMT_FASTA, FMT_FASTQ, FMT_PLAIN = 0, 1, 2
KEYS_DUMP, KEYS_TABLE = 0, 1  # kc_lookup* key layouts (KC_KEYS_DUMP / KC_KEYS_TABLE)
NO_KMER = 0xFFFFFFFF  # kc_text_counts*: no k-mer starts at this position (KC_NO_KMER)
# kc_seq_stat (include/kc_api.h), 32 bytes
SEQ_STAT_DTYPE = np.dtype([("windows", "<u4"), ("present", "<u4"), ("solid", "<u4"), ("min", "<u4"),
                           ("median", "<u4"), ("max", "<u4"), ("sum", "<u8")])
# kc_correct_stat (include/kc_api.h), 16 bytes
CORRECT_STAT_DTYPE = np.dtype([("candidates", "<u4"), ("corrected", "<u4"), ("ambiguous", "<u4"), ("dropped", "<u4")])

# Public C-ABI symbols (include/kc_api.h); tests check every one is exported.
EXPORTS = (
    "kc_create", "kc_destroy", "kc_last_error", "kc_bloom_chunk", "kc_bloom_finalize",
    "kc_count_chunk", "kc_bloom_device", "kc_count_device", "kc_sync", "kc_finish", "kc_dump",
    "kc_write", "kc_key_words", "kc_free", "kc_plan_chunks", "kc_synth_bytes", "kc_synth_device",
    "kc_reset", "kc_profile", "kc_get_timing", "kc_route_device", "kc_insert_keys_device",
    "kc_route_table_device", "kc_route_hint", "kc_insert_counts_device", "kc_clear_table", "kc_insert_counts_runs_device",
    "kc_xxh64", "kc_bloom_info", "kc_bloom_read", "kc_bloom_write", "kc_synth_skew_device",
    "kc_table_size_reference", "kc_bloom_get_device", "kc_bloom_merge_device", "kc_bloom_set_device",
    "kc_bloom_estimate", "kc_compact", "kc_compact_dump", "kc_compact_lookup", "kc_compact_read", "kc_size_table",
    "kc_estimate_distinct_device", "kc_bloom_records_device", "kc_count_records_device", "kc_plan_chunks_device",
    "kc_output_digest", "kc_route_superkmers_device", "kc_count_packed_device", "kc_bloom_packed_device",
    "kc_packed_windows_device",
    "kc_lookup_device", "kc_lookup", "kc_histogram",
    "kc_text_counts_device", "kc_text_counts", "kc_seq_stats_device", "kc_seq_stats",
    "kc_table_op_device", "kc_table_op",
    "kc_correct_device", "kc_correct",
    "kc_neighbors_device", "kc_neighbors", "kc_graph_device", "kc_graph",
    "kc_unitigs_device", "kc_unitigs",
    "kc_unitig_graph_device", "kc_unitig_graph",
    "kc_read_paths_device", "kc_read_paths",
    "kc_clean_device", "kc_clean",
    "kc_pop_bubbles_device", "kc_pop_bubbles", "kc_cut_weak_device", "kc_cut_weak",
)
# kc_graph* node flags (KC_GRAPH_*): bits 0-7 the edges -- bit y: canon(c[1:] + y) is a node (side
# R), bit 4 + y: canon(y + c[:-1]) is a node (side L) -- then the two unitig links and the node bit
GRAPH_LINK_R, GRAPH_LINK_L, GRAPH_NODE = 0x0100, 0x0200, 0x8000
UNITIG_CIRCULAR = 1  # kc_unitig.flags (KC_UNITIG_CIRCULAR)
# kc_unitig_edge.flags (KC_EDGE_*): the edge leaves `from` through the start of its string, enters
# `to` at the end of its string
EDGE_FROM_REV, EDGE_TO_REV = 1, 2
# kc_unitig_edge (include/kc_api.h), 16 bytes
EDGE_DTYPE = np.dtype([("from", "<u4"), ("to", "<u4"), ("flags", "<u4"), ("reserved", "<u4")])
# kc_path_run.flags (KC_RUN_*): the run reads its unitig as U-; the window before its first is located too
RUN_REV, RUN_JOINED = 1, 2
NO_UNITIG = 0xFFFFFFFF  # KC_NO_UNITIG
# kc_path_run and kc_path_seq (include/kc_api.h), 32 bytes each
RUN_DTYPE = np.dtype([("text_pos", "<u8"), ("seq", "<u4"), ("windows", "<u4"), ("unitig", "<u4"), ("pos", "<u4"),
                      ("flags", "<u4"), ("reserved", "<u4")])
PATH_SEQ_DTYPE = np.dtype([("first_run", "<u8"), ("windows", "<u4"), ("located", "<u4"), ("runs", "<u4"),
                           ("chains", "<u4"), ("longest_chain", "<u4"), ("reserved", "<u4")])
# kc_table_op* operations (KC_OP_*): on the raw counts ca, cb of a key in a and in b
OP_INTERSECT_MIN, OP_INTERSECT_SUM, OP_INTERSECT_LEFT, OP_SUBTRACT, OP_COUNTS_SUBTRACT, OP_UNION_SUM, OP_UNION_MAX = range(7)
OP_NAMES = {"intersect-min": OP_INTERSECT_MIN, "intersect-sum": OP_INTERSECT_SUM, "intersect-left": OP_INTERSECT_LEFT,
            "subtract": OP_SUBTRACT, "counts-subtract": OP_COUNTS_SUBTRACT, "union-sum": OP_UNION_SUM,
            "union-max": OP_UNION_MAX}


def unitig_strings(records, bases, k: int) -> List[str]:
    """the strings of unitig records (n, 4) {offset, n_nodes, ...}: bases[offset : offset + n_nodes + k - 1]"""
    b = np.ascontiguousarray(bases, dtype=np.uint8).tobytes()
    return [b[int(o):int(o) + int(n) + k - 1].decode("ascii") for o, n in np.asarray(records)[:, :2].tolist()]


def gfa_lines(records, bases, edges, k: int) -> List[str]:
    """The compacted graph as GFA 1.0 lines (without line ends), what the CLI's --gfa writes: the
    header, "S <i> <bases> LN:i:<n + k - 1> KC:i:<count_sum>" per unitig record in record order,
    "L <from> <+|-> <to> <+|-> <k - 1>M" per edge (EDGE_DTYPE) in the edges' order, and the two
    closing links "L i + i +" and "L i - i -" of every circular unitig, in record order."""
    records = np.asarray(records, dtype=np.uint64).reshape(-1, 4)
    edges = np.asarray(edges, dtype=EDGE_DTYPE)
    out = ["H\tVN:Z:1.0"]
    for i, (s, (_, _, total, _)) in enumerate(zip(unitig_strings(records, bases, k), records.tolist())):
        out.append(f"S\t{i}\t{s}\tLN:i:{len(s)}\tKC:i:{total}")
    for a, b, fl in zip(edges["from"].tolist(), edges["to"].tolist(), edges["flags"].tolist()):
        out.append(f"L\t{a}\t{'-' if fl & EDGE_FROM_REV else '+'}\t{b}\t{'-' if fl & EDGE_TO_REV else '+'}\t{k - 1}M")
    for i in np.flatnonzero(records[:, 3] & np.uint64(UNITIG_CIRCULAR)).tolist():
        out += [f"L\t{i}\t{o}\t{i}\t{o}\t{k - 1}M" for o in "+-"]
    return out


def gaf_lines(names, seqs, records, runs, k: int) -> List[str]:
    """The read paths as GAF lines (without line ends), what the CLI's --paths-out writes: one line
    per chain in run order, "name qlen qstart qend + path plen pstart pend matches alnlen 255
    cg:Z:<alnlen>=".  names and seqs: the sequences of the read_paths call (their text joined by
    pack_sequences); records, runs: its records and RUN_DTYPE runs.  path is ">i" or "<i" per
    segment visit, a run that goes round a circle visiting it once per lap; qend - qstart = the
    chain's windows + k - 1 = matches = alnlen = pend - pstart; plen is the sum of the visited
    segments' lengths minus k - 1 per junction."""
    records = np.asarray(records, dtype=np.uint64).reshape(-1, 4)
    runs = np.asarray(runs, dtype=RUN_DTYPE)
    starts = np.zeros(len(seqs) + 1, dtype=np.int64)
    if len(seqs):
        starts[1:] = np.cumsum([len(s_) + 1 for s_ in seqs])
    out = []
    chain = None  # [seq, qstart, path, plen, pstart, windows, visits]
    def flush():
        if chain is None:
            return
        i, qstart, path, plen, pstart, windows, _ = chain
        aln = windows + k - 1
        out.append(f"{names[i]}\t{len(seqs[i])}\t{qstart}\t{qstart + aln}\t+\t{path}\t{plen}\t{pstart}\t{pstart + aln}"
                   f"\t{aln}\t{aln}\t255\tcg:Z:{aln}=")
    for r in runs.tolist():
        text_pos, i, windows, u, q, flags = r[:6]
        n_nodes, circ = int(records[u, 1]), bool(int(records[u, 3]) & UNITIG_CIRCULAR)
        if not flags & RUN_JOINED or chain is None:
            flush()
            chain = [i, text_pos - int(starts[i]), "", 0, q, 0, 0]
        laps = (q + windows - 1) // n_nodes + 1 if circ else 1
        for _ in range(laps):
            chain[2] += ("<" if flags & RUN_REV else ">") + str(u)
            chain[3] += n_nodes + k - 1 - (k - 1 if chain[6] else 0)
            chain[6] += 1
        chain[5] += windows
    flush()
    return out


class KcError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


class kc_config(ctypes.Structure):
    _fields_ = [
        ("k", ctypes.c_int32), ("mode", ctypes.c_int32), ("bf_enable", ctypes.c_int32),
        ("device", ctypes.c_int32), ("table_slots", ctypes.c_uint64), ("est_unique", ctypes.c_uint64),
        ("fpr", ctypes.c_double), ("min_abundance", ctypes.c_uint64), ("batch_bytes", ctypes.c_uint64),
    ]


class kc_chunk(ctypes.Structure):
    _fields_ = [("off", ctypes.c_uint64), ("len", ctypes.c_uint64),
                ("broken_header", ctypes.c_int32), ("pad", ctypes.c_int32)]


class kc_timing(ctypes.Structure):
    _fields_ = [("gather_ms", ctypes.c_double), ("tokenize_ms", ctypes.c_double), ("count_ms", ctypes.c_double),
                ("launches", ctypes.c_uint64), ("symbols", ctypes.c_uint64)]


class kc_synth_skew(ctypes.Structure):
    _fields_ = [("homo_frac", ctypes.c_double), ("dinuc_frac", ctypes.c_double),
                ("repeat_len", ctypes.c_uint32), ("repeat_copies", ctypes.c_uint32)]


class kc_compact_info(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("slots", "kmers", "chain_starts", "bytes", "table_bytes")]


class kc_digest(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("lines", "count_sum", "hash_sum", "hash_xor")]


class kc_op_desc(ctypes.Structure):  # 24 bytes
    _fields_ = [("op", ctypes.c_int32), ("a_min", ctypes.c_uint32), ("a_max", ctypes.c_uint32),
                ("b_min", ctypes.c_uint32), ("b_max", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class kc_op_stats(ctypes.Structure):  # 40 bytes
    _fields_ = [(n, ctypes.c_uint64) for n in ("a_keys", "both", "b_only", "out_keys", "out_sum")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class kc_graph_stats(ctypes.Structure):  # 80 bytes
    _fields_ = [(n, ctypes.c_uint64) for n in ("nodes", "edge_ends", "link_ends", "isolated", "palindromes")] + \
               [("side_degree", ctypes.c_uint64 * 5)]

    def as_dict(self) -> dict:
        """the ten statistics, side_degree as a list, plus open_unitigs = nodes - link_ends / 2"""
        d = {n: int(getattr(self, n)) for n, _ in self._fields_[:5]}
        d["side_degree"] = [int(x) for x in self.side_degree]
        d["open_unitigs"] = d["nodes"] - d["link_ends"] // 2
        return d


class kc_unitig(ctypes.Structure):  # 32 bytes
    _fields_ = [(n, ctypes.c_uint64) for n in ("offset", "n_nodes", "count_sum", "flags")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class kc_unitig_stats(ctypes.Structure):  # 40 bytes
    _fields_ = [(n, ctypes.c_uint64) for n in ("unitigs", "circular", "nodes", "bases", "max_nodes")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class kc_unitig_edge(ctypes.Structure):  # 16 bytes
    _fields_ = [(n, ctypes.c_uint32) for n in ("from", "to", "flags", "reserved")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class kc_cdbg_stats(ctypes.Structure):  # 64 bytes
    _fields_ = [(n, ctypes.c_uint64) for n in ("unitigs", "circular", "nodes", "bases", "max_nodes", "edges",
                                               "dead_ends", "reserved")]

    def as_dict(self) -> dict:
        """the seven statistics (without the reserved word)"""
        return {n: int(getattr(self, n)) for n, _ in self._fields_[:7]}


class kc_path_run(ctypes.Structure):  # 32 bytes
    _fields_ = [("text_pos", ctypes.c_uint64), ("seq", ctypes.c_uint32), ("windows", ctypes.c_uint32),
                ("unitig", ctypes.c_uint32), ("pos", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class kc_path_seq(ctypes.Structure):  # 32 bytes
    _fields_ = [("first_run", ctypes.c_uint64), ("windows", ctypes.c_uint32), ("located", ctypes.c_uint32),
                ("runs", ctypes.c_uint32), ("chains", ctypes.c_uint32), ("longest_chain", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32)]


class kc_path_stats(ctypes.Structure):  # 64 bytes
    _fields_ = [("seqs", ctypes.c_uint64), ("windows", ctypes.c_uint64), ("located", ctypes.c_uint64),
                ("runs", ctypes.c_uint64), ("chains", ctypes.c_uint64), ("threaded", ctypes.c_uint64),
                ("reserved", ctypes.c_uint64 * 2)]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n in ("seqs", "windows", "located", "runs", "chains", "threaded")}


class kc_clean_desc(ctypes.Structure):  # 24 bytes
    _fields_ = [(n, ctypes.c_uint32) for n in ("min_count", "max_count", "tip_max_nodes", "iso_max_nodes", "max_mean",
                                               "reserved")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class kc_clean_stats(ctypes.Structure):  # 64 bytes
    _fields_ = [(n, ctypes.c_uint64) for n in ("unitigs", "nodes", "tips", "tip_nodes", "isolated", "isolated_nodes",
                                               "out_keys", "out_sum")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class kc_bubble_desc(ctypes.Structure):  # 24 bytes
    _fields_ = [(n, ctypes.c_uint32) for n in ("min_count", "max_count", "max_nodes", "max_diff", "max_mean", "reserved")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class kc_bubble_stats(ctypes.Structure):  # 64 bytes
    _fields_ = [(n, ctypes.c_uint64) for n in ("unitigs", "nodes", "branches", "parallel", "popped", "popped_nodes",
                                               "out_keys", "out_sum")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class kc_weak_desc(ctypes.Structure):  # 24 bytes
    _fields_ = [(n, ctypes.c_uint32) for n in ("min_count", "max_count", "max_nodes", "ratio_permille", "max_mean",
                                               "reserved")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class kc_weak_stats(ctypes.Structure):  # 64 bytes
    _fields_ = [(n, ctypes.c_uint64) for n in ("unitigs", "nodes", "interior", "weak", "cut", "cut_nodes", "out_keys",
                                               "out_sum")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class kc_correct_stat(ctypes.Structure):  # 16 bytes
    _fields_ = [(n, ctypes.c_uint32) for n in ("candidates", "corrected", "ambiguous", "dropped")]


class kc_stats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in (
        "windows", "inserted", "distinct", "table_slots", "bf_windows", "bf_bits", "new_in_first",
        "new_in_second", "failed_in_first", "chunks", "bytes", "part_fallbacks", "spilled", "heavy_records",
        "reused_passes", "reuse_level", "route_counts_kept", "deferred_level3")]

    def as_dict(self) -> dict:
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


_lib: Optional[ctypes.CDLL] = None


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libkc.so (raises if it is missing: there is no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise FileNotFoundError(
            f"{path} not built; run `make -C {PKG_ROOT}` or __graft_entry__.build()")
    # PyTorch-ROCm wheels ship their own libamdhip64.so.7.  If torch is around, load
    # it first so that libkc.so binds to that same runtime (one HIP runtime per
    # process; device pointers and streams are then shared with torch).  Without
    # torch, libkc.so uses /opt/rocm's runtime through its RUNPATH.
    try:
        import torch  # noqa: F401
        if torch.cuda.is_available():
            torch.cuda.init()
    except ImportError:
        pass
    lib = ctypes.CDLL(path)
    P, U64, I32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    sig = {
        "kc_create": (I32, [ctypes.POINTER(kc_config), ctypes.POINTER(P)]),
        "kc_destroy": (None, [P]),
        "kc_last_error": (ctypes.c_char_p, [P]),
        "kc_bloom_chunk": (I32, [P, P, ctypes.c_size_t, I32, I32]),
        "kc_bloom_finalize": (I32, [P, ctypes.POINTER(U64)]),
        "kc_count_chunk": (I32, [P, P, ctypes.c_size_t, I32, I32]),
        "kc_bloom_device": (I32, [P, P, ctypes.POINTER(kc_chunk), ctypes.c_size_t, I32, P]),
        "kc_count_device": (I32, [P, P, ctypes.POINTER(kc_chunk), ctypes.c_size_t, I32, P]),
        "kc_estimate_distinct_device": (I32, [P, P, ctypes.POINTER(kc_chunk), ctypes.c_size_t, I32, P,
                                              ctypes.POINTER(ctypes.c_double)]),
        "kc_size_table": (I32, [P, U64]),
        "kc_route_superkmers_device": (I32, [P, P, ctypes.POINTER(kc_chunk), ctypes.c_size_t, I32, ctypes.c_uint32,
                                             I32, P, P, U64, ctypes.POINTER(U64), ctypes.POINTER(U64), P]),
        "kc_count_packed_device": (I32, [P, P, P, U64, U64, P]),
        "kc_bloom_packed_device": (I32, [P, P, P, U64, U64, P]),
        "kc_packed_windows_device": (I32, [P, P, P, U64, P, ctypes.POINTER(ctypes.c_uint64)]),
        "kc_sync": (I32, [P]),
        "kc_finish": (I32, [P, ctypes.POINTER(kc_stats)]),
        "kc_dump": (I32, [P, ctypes.POINTER(ctypes.POINTER(U64)), ctypes.POINTER(U64)]),
        "kc_write": (I32, [P, ctypes.c_char_p]),
        "kc_output_digest": (I32, [P, ctypes.POINTER(kc_digest)]),
        "kc_key_words": (I32, [P]),
        "kc_free": (None, [P]),
        "kc_plan_chunks": (I32, [P, U64, I32, U64, I32, ctypes.POINTER(ctypes.POINTER(kc_chunk)),
                                 ctypes.POINTER(U64)]),
        "kc_plan_chunks_device": (I32, [P, U64, I32, U64, I32, ctypes.POINTER(ctypes.POINTER(kc_chunk)),
                                 ctypes.POINTER(U64)]),
        "kc_synth_bytes": (U64, [U64, U64, ctypes.c_uint32, ctypes.c_uint32]),
        "kc_reset": (I32, [P]),
        "kc_clear_table": (I32, [P]),
        "kc_insert_counts_runs_device": (I32, [P, P, ctypes.POINTER(U64), ctypes.c_uint32, P]),
        "kc_route_device": (I32, [P, P, ctypes.POINTER(kc_chunk), ctypes.c_size_t, I32, ctypes.c_uint32, P, U64,
                                  ctypes.POINTER(U64), P]),
        "kc_insert_keys_device": (I32, [P, P, U64, P]),
        "kc_route_table_device": (I32, [P, ctypes.c_uint32, P, U64, P, P]),
        "kc_route_hint": (I32, [P, ctypes.c_uint32]),
        "kc_insert_counts_device": (I32, [P, P, U64, P]),
        "kc_bloom_records_device": (I32, [P, P, U64, P]),
        "kc_count_records_device": (I32, [P, P, U64, P]),
        "kc_profile": (I32, [P, I32]),
        "kc_get_timing": (I32, [P, ctypes.POINTER(kc_timing)]),
        "kc_synth_device": (I32, [P, U64, U64, U64, U64, ctypes.c_uint32, ctypes.c_uint32,
                                  ctypes.c_double, ctypes.c_double, P]),
        "kc_xxh64": (I32, [P, P, U64, P]),
        "kc_table_size_reference": (U64, [U64]),
        "kc_synth_skew_device": (I32, [P, U64, U64, U64, U64, ctypes.c_uint32, ctypes.c_uint32,
                                       ctypes.c_double, ctypes.c_double, ctypes.POINTER(kc_synth_skew), P]),
        "kc_bloom_info": (I32, [P, ctypes.POINTER(U64), ctypes.POINTER(U64), ctypes.POINTER(I32),
                                ctypes.POINTER(I32), ctypes.POINTER(I32)]),
        "kc_bloom_read": (I32, [P, P, U64]),
        "kc_bloom_write": (I32, [P, P, U64]),
        "kc_bloom_get_device": (I32, [P, P, U64, U64, P]),
        "kc_bloom_merge_device": (I32, [P, P, ctypes.c_uint32, U64, P, P]),
        "kc_bloom_set_device": (I32, [P, P, U64, ctypes.POINTER(U64), P]),
        "kc_bloom_estimate": (I32, [P, ctypes.POINTER(U64), P]),
        "kc_compact": (I32, [P, ctypes.c_double, ctypes.POINTER(kc_compact_info)]),
        "kc_compact_dump": (I32, [P, ctypes.POINTER(ctypes.POINTER(U64)), ctypes.POINTER(U64), ctypes.POINTER(U64),
                                  ctypes.POINTER(ctypes.c_double)]),
        "kc_compact_lookup": (I32, [P, P, U64, P]),
        "kc_compact_read": (I32, [P, P, U64, P, U64]),
        "kc_lookup_device": (I32, [P, P, U64, I32, P, P]),
        "kc_lookup": (I32, [P, P, U64, I32, P]),
        "kc_histogram": (I32, [P, P, ctypes.c_uint32]),
        "kc_text_counts_device": (I32, [P, P, U64, P, P]),
        "kc_text_counts": (I32, [P, P, U64, P]),
        "kc_seq_stats_device": (I32, [P, P, U64, P, U64, ctypes.c_uint32, P, P]),
        "kc_seq_stats": (I32, [P, P, U64, P, U64, ctypes.c_uint32, P]),
        "kc_correct_device": (I32, [P, P, U64, P, U64, ctypes.c_uint32, P, P, P]),
        "kc_correct": (I32, [P, P, U64, P, U64, ctypes.c_uint32, P, P]),
        "kc_table_op_device": (I32, [P, P, P, ctypes.POINTER(kc_op_desc), P, P]),
        "kc_table_op": (I32, [P, P, P, ctypes.POINTER(kc_op_desc), ctypes.POINTER(kc_op_stats)]),
        "kc_neighbors_device": (I32, [P, P, U64, I32, P, P]),
        "kc_neighbors": (I32, [P, P, U64, I32, P]),
        "kc_graph_device": (I32, [P, ctypes.c_uint32, ctypes.c_uint32, P, U64, P, P, P]),
        "kc_graph": (I32, [P, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.POINTER(U64)),
                           ctypes.POINTER(U64), ctypes.POINTER(kc_graph_stats)]),
        "kc_unitigs_device": (I32, [P, ctypes.c_uint32, ctypes.c_uint32, P, U64, P, U64, P, P]),
        "kc_unitigs": (I32, [P, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.POINTER(kc_unitig)),
                             ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), ctypes.POINTER(kc_unitig_stats)]),
        "kc_clean_device": (I32, [P, P, ctypes.POINTER(kc_clean_desc), P, P]),
        "kc_clean": (I32, [P, P, ctypes.POINTER(kc_clean_desc), ctypes.POINTER(kc_clean_stats)]),
        "kc_pop_bubbles_device": (I32, [P, P, ctypes.POINTER(kc_bubble_desc), P, P]),
        "kc_pop_bubbles": (I32, [P, P, ctypes.POINTER(kc_bubble_desc), ctypes.POINTER(kc_bubble_stats)]),
        "kc_cut_weak_device": (I32, [P, P, ctypes.POINTER(kc_weak_desc), P, P]),
        "kc_cut_weak": (I32, [P, P, ctypes.POINTER(kc_weak_desc), ctypes.POINTER(kc_weak_stats)]),
        "kc_unitig_graph_device": (I32, [P, ctypes.c_uint32, ctypes.c_uint32, P, U64, P, U64, P, U64, P, P]),
        "kc_unitig_graph": (I32, [P, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.POINTER(kc_unitig)),
                                  ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)),
                                  ctypes.POINTER(ctypes.POINTER(kc_unitig_edge)), ctypes.POINTER(kc_cdbg_stats)]),
        "kc_read_paths_device": (I32, [P, ctypes.c_uint32, ctypes.c_uint32, P, U64, P, U64, P, U64, P, P, U64, P, U64, P, U64,
                                       P, P, P]),
        "kc_read_paths": (I32, [P, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(ctypes.POINTER(kc_unitig)),
                                ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)),
                                ctypes.POINTER(ctypes.POINTER(kc_unitig_edge)), ctypes.POINTER(kc_cdbg_stats), P, U64, P, U64,
                                ctypes.POINTER(ctypes.POINTER(kc_path_run)), ctypes.POINTER(ctypes.POINTER(kc_path_seq)),
                                ctypes.POINTER(kc_path_stats)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


MAX_K = 479  # include/kc_api.h KC_MAX_K


def words_for_k(k: int) -> int:
    return k // 32 + 1


def xxh64_device(values: Sequence[int], seeds: Sequence[int]) -> List[int]:
    """XXH64(&v, 8, seed) of each pair by the device function of the reference-layout
    Bloom passes (kc_xxh64 test hook)."""
    lib = load_library()
    v = np.ascontiguousarray(values, dtype=np.uint64)
    sd = np.ascontiguousarray(seeds, dtype=np.uint64)
    out = np.zeros(v.size, dtype=np.uint64)
    rc = lib.kc_xxh64(v.ctypes.data, sd.ctypes.data, v.size, out.ctypes.data)
    if rc:
        raise KcError(rc, "kc_xxh64")
    return [int(x) for x in out]


def detect_format(path: str, first_byte: int) -> int:
    """file_format (main.cpp:27-68) on an uncompressed image: returns FMT_* or raises."""
    ext = os.path.splitext(path)[1]
    if ext in (".fasta", ".fa"):
        ok, fmt = first_byte == ord(">"), FMT_FASTA
    elif ext in (".fastq", ".fq"):
        ok, fmt = first_byte == ord("@"), FMT_FASTQ
    else:
        ok, fmt = first_byte in b"actgACGT", FMT_PLAIN
    if not ok:
        raise ValueError(f"Input file {path} is ill-formed")
    return fmt


def plan_chunks(image: bytes, k: int, fmt: int, chunk_size: int = 0) -> List[Tuple[int, int, int]]:
    """Reference chunk table (off, len, broken_header) of a file image."""
    lib = load_library()
    buf = ctypes.create_string_buffer(bytes(image), len(image)) if len(image) else None
    out = ctypes.POINTER(kc_chunk)()
    n = ctypes.c_uint64()
    rc = lib.kc_plan_chunks(buf, len(image), k, chunk_size, fmt, ctypes.byref(out), ctypes.byref(n))
    if rc:
        raise KcError(rc, "kc_plan_chunks")
    res = [(out[i].off, out[i].len, out[i].broken_header) for i in range(n.value)]
    lib.kc_free(out)
    return res


def plan_chunks_device(dev_ptr: int, size: int, k: int, fmt: int, chunk_size: int = 0) -> List[Tuple[int, int, int]]:
    """plan_chunks for an image in device memory (kc_plan_chunks_device: only the bytes around
    chunk ends are copied to the host)."""
    lib = load_library()
    out = ctypes.POINTER(kc_chunk)()
    n = ctypes.c_uint64()
    rc = lib.kc_plan_chunks_device(ctypes.c_void_p(dev_ptr or None), size, k, chunk_size, fmt, ctypes.byref(out),
                                   ctypes.byref(n))
    if rc:
        raise KcError(rc, "kc_plan_chunks_device")
    res = [(out[i].off, out[i].len, out[i].broken_header) for i in range(n.value)]
    lib.kc_free(out)
    return res


def decode_records(records: np.ndarray, k: int) -> List[Tuple[str, int]]:
    """(W+1)-word records -> [(kmer string, T(c))] (test helper, vectorised)."""
    W = words_for_k(k)
    recs = records.reshape(-1, W + 1)
    n = recs.shape[0]
    chars = np.empty((n, k), dtype=np.uint8)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    for j in range(k):
        bit = 2 * (k - 1 - j)
        word = W - 1 - bit // 64
        chars[:, j] = lut[(recs[:, word] >> np.uint64(bit % 64)) & np.uint64(3)]
    strs = [bytes(r).decode() for r in chars]
    return list(zip(strs, (int(c) for c in recs[:, W])))


def encode_kmers(strings: Sequence[str], k: int) -> np.ndarray:
    """k-mer strings -> (n, W) uint64 keys in dump()'s key layout (the inverse of decode_records'
    key part; the strand is kept as given).  A/C/G/T in upper or lower case; anything else, or a
    string of another length, raises ValueError."""
    W = words_for_k(k)
    n = len(strings)
    keys = np.zeros((n, W), dtype=np.uint64)
    if n == 0:
        return keys
    for s_ in strings:
        if len(s_) != k:
            raise ValueError(f"not a {k}-mer: {s_!r}")
    try:
        raw = np.frombuffer("".join(strings).encode("ascii"), dtype=np.uint8).reshape(n, k)
    except UnicodeEncodeError as e:
        raise ValueError(f"not a nucleotide string: {e}") from None
    lut = np.full(256, 255, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        lut[ch] = lut[ch + 32] = i
    codes = lut[raw]
    if (codes > 3).any():
        bad = int(np.argwhere(codes > 3)[0][0])
        raise ValueError(f"not A/C/G/T: {strings[bad]!r}")
    for j in range(k):
        bit = 2 * (k - 1 - j)
        keys[:, W - 1 - bit // 64] |= codes[:, j].astype(np.uint64) << np.uint64(bit % 64)
    return keys


def pack_sequences(seqs: Sequence) -> Tuple[bytes, np.ndarray]:
    """Sequences (str or bytes) -> (text, offsets) for seq_stats / kc_seq_stats: the sequences joined
    with one newline each (a break byte), offsets[i] .. offsets[i + 1] - 1 being sequence i and its
    newline; uint64 offsets of len(seqs) + 1 entries, so the last is len(text)."""
    parts = [s_.encode("ascii") if isinstance(s_, str) else bytes(s_) for s_ in seqs]
    offsets = np.zeros(len(parts) + 1, dtype=np.uint64)
    if parts:
        offsets[1:] = np.cumsum([len(p_) + 1 for p_ in parts], dtype=np.uint64)
    return b"".join(p_ + b"\n" for p_ in parts), offsets


@dataclass
class Config:
    k: int
    mode: int = 2
    table_slots: int = 1 << 20
    bf_enable: bool = False
    est_unique: int = 0
    fpr: float = 0.01
    min_abundance: int = 2
    device: int = 0
    batch_bytes: int = 0

    def to_c(self) -> kc_config:
        return kc_config(self.k, self.mode, int(self.bf_enable), self.device, self.table_slots,
                         self.est_unique, self.fpr, self.min_abundance, self.batch_bytes)


class KmerCounter:
    """One device table (+ optional double Bloom filter) behind the C ABI."""

    def __init__(self, cfg: Config):
        self.lib = load_library()
        self.cfg = cfg
        self._ctx = ctypes.c_void_p()
        c = cfg.to_c()
        rc = self.lib.kc_create(ctypes.byref(c), ctypes.byref(self._ctx))
        if rc:
            raise KcError(rc, self.lib.kc_last_error(None).decode())

    # -- lifecycle
    def close(self):
        if self._ctx:
            self.lib.kc_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int, what: str):
        if rc:
            raise KcError(rc, f"{what}: {self.lib.kc_last_error(self._ctx).decode()}")

    # -- passes over host chunks
    def bloom_chunk(self, buf: bytes, fmt: int, broken_header: bool = False):
        self._chk(self.lib.kc_bloom_chunk(self._ctx, buf, len(buf), fmt, int(broken_header)), "kc_bloom_chunk")

    def bloom_finalize(self) -> int:
        n = ctypes.c_uint64()
        self._chk(self.lib.kc_bloom_finalize(self._ctx, ctypes.byref(n)), "kc_bloom_finalize")
        return n.value

    def count_chunk(self, buf: bytes, fmt: int, broken_header: bool = False):
        self._chk(self.lib.kc_count_chunk(self._ctx, buf, len(buf), fmt, int(broken_header)), "kc_count_chunk")

    # -- passes over a device-resident image (e.g. a torch uint8 CUDA tensor's data_ptr)
    @staticmethod
    def _chunk_array(chunks: Sequence[Tuple[int, int, int]]):
        arr = (kc_chunk * max(1, len(chunks)))()
        for i, (o, l, b) in enumerate(chunks):
            arr[i].off, arr[i].len, arr[i].broken_header = o, l, b
        return arr

    def bloom_device(self, dev_ptr: int, chunks, fmt: int, stream: int = 0):
        arr = self._chunk_array(chunks)
        self._chk(self.lib.kc_bloom_device(self._ctx, ctypes.c_void_p(dev_ptr), arr, len(chunks), fmt,
                                           ctypes.c_void_p(stream or None)), "kc_bloom_device")

    def count_device(self, dev_ptr: int, chunks, fmt: int, stream: int = 0):
        arr = self._chunk_array(chunks)
        self._chk(self.lib.kc_count_device(self._ctx, ctypes.c_void_p(dev_ptr), arr, len(chunks), fmt,
                                           ctypes.c_void_p(stream or None)), "kc_count_device")

    def estimate_distinct_device(self, dev_ptr: int, chunks, fmt: int, stream: int = 0) -> float:
        """HyperLogLog estimate of the image's distinct canonical k-mers (2^14 registers, ~0.8 %
        standard error); counts nothing.  For sizing a table before counting."""
        arr = self._chunk_array(chunks)
        est = ctypes.c_double(0.0)
        self._chk(self.lib.kc_estimate_distinct_device(self._ctx, ctypes.c_void_p(dev_ptr), arr, len(chunks), fmt,
                                                       ctypes.c_void_p(stream or None), ctypes.byref(est)),
                  "kc_estimate_distinct_device")
        return est.value

    def size_table(self, slots: int):
        """Size the table of the job about to be counted for `slots` k-mers (e.g. 1.1 x the distinct
        estimate) instead of -s, which stays the job's reference capacity; 0 = back to -s
        (kc_size_table: after create / reset, before the first counting pass)."""
        self._chk(self.lib.kc_size_table(self._ctx, int(slots)), "kc_size_table")

    def route_superkmers_device(self, dev_ptr: int, chunks, fmt: int, nshards: int, pk_ptr: int = 0, bk_ptr: int = 0,
                                cap_words: int = 0, m: int = 0, stream: int = 0):
        """Super-k-mers of a device image, per owner (canonical-minimizer owner, kc_api.h): region o of
        pk / bk (cap_words words each, at o * cap_words) receives owner o's packed stream.  Returns
        (words per owner, windows per owner); cap_words = 0 only sizes them.  Raises KcError
        (KC_ERR_NOMEM) when a region is too small -- its .words holds the sizes needed."""
        arr = self._chunk_array(chunks)
        words = (ctypes.c_uint64 * nshards)()
        wins = (ctypes.c_uint64 * nshards)()
        rc = self.lib.kc_route_superkmers_device(self._ctx, ctypes.c_void_p(dev_ptr), arr, len(chunks), fmt, nshards, m,
                                                 ctypes.c_void_p(pk_ptr or None), ctypes.c_void_p(bk_ptr or None),
                                                 cap_words, words, wins, ctypes.c_void_p(stream or None))
        if rc:
            err = KcError(rc, f"kc_route_superkmers_device: {self.lib.kc_last_error(self._ctx).decode()}")
            err.words = list(words)
            raise err
        return list(words), list(wins)

    def count_packed_device(self, pk_ptr: int, bk_ptr: int, n_words: int, windows: int = 0, stream: int = 0):
        """Counts the windows of a packed symbol stream in HBM (e.g. received super-k-mers)."""
        self._chk(self.lib.kc_count_packed_device(self._ctx, ctypes.c_void_p(pk_ptr or None),
                                                  ctypes.c_void_p(bk_ptr or None), n_words, windows,
                                                  ctypes.c_void_p(stream or None)), "kc_count_packed_device")

    def bloom_packed_device(self, pk_ptr: int, bk_ptr: int, n_words: int, windows: int = 0, stream: int = 0):
        """Bloom pass 1 over a packed symbol stream in HBM."""
        self._chk(self.lib.kc_bloom_packed_device(self._ctx, ctypes.c_void_p(pk_ptr or None),
                                                  ctypes.c_void_p(bk_ptr or None), n_words, windows,
                                                  ctypes.c_void_p(stream or None)), "kc_bloom_packed_device")

    def packed_windows_device(self, pk_ptr: int, bk_ptr: int, n_words: int, stream: int = 0) -> int:
        """The windows of a packed symbol stream in HBM, counted from its break words: the honest
        value of the `windows` hint of count_packed_device / bloom_packed_device."""
        n = ctypes.c_uint64(0)
        self._chk(self.lib.kc_packed_windows_device(self._ctx, ctypes.c_void_p(pk_ptr or None),
                                                    ctypes.c_void_p(bk_ptr or None), n_words,
                                                    ctypes.c_void_p(stream or None), ctypes.byref(n)),
                  "kc_packed_windows_device")
        return int(n.value)

    def route_device(self, dev_ptr: int, chunks, fmt: int, nshards: int, out_ptr: int, out_capacity: int,
                     stream: int = 0) -> List[int]:
        """Table keys of the image's windows grouped by owner shard into out_ptr; returns counts."""
        arr = self._chunk_array(chunks)
        counts = (ctypes.c_uint64 * nshards)()
        self._chk(self.lib.kc_route_device(self._ctx, ctypes.c_void_p(dev_ptr), arr, len(chunks), fmt, nshards,
                                           ctypes.c_void_p(out_ptr), out_capacity, counts,
                                           ctypes.c_void_p(stream or None)), "kc_route_device")
        return [int(x) for x in counts]

    def insert_keys_device(self, keys_ptr: int, n_keys: int, stream: int = 0):
        self._chk(self.lib.kc_insert_keys_device(self._ctx, ctypes.c_void_p(keys_ptr), n_keys,
                                                 ctypes.c_void_p(stream or None)), "kc_insert_keys_device")

    def route_table_device(self, nshards: int, out_ptr: int, out_capacity: int, stream: int = 0) -> List[int]:
        """The table's occupied slots as {W table-key words, raw count} records grouped by
        owner shard into out_ptr (0 = count only); returns the per-owner record counts."""
        counts = (ctypes.c_uint64 * nshards)()
        self._chk(self.lib.kc_route_table_device(self._ctx, nshards, ctypes.c_void_p(out_ptr or None), out_capacity,
                                                 counts, ctypes.c_void_p(stream or None)), "kc_route_table_device")
        return [int(x) for x in counts]

    def route_hint(self, nshards: int):
        """The table will be routed to nshards owners: the counting passes keep the per-block
        owner counts so route_table_device runs no count pass (include/kc_api.h kc_route_hint)."""
        self._chk(self.lib.kc_route_hint(self._ctx, nshards), "kc_route_hint")

    def bloom_records_device(self, rec_ptr: int, n_records: int, stream: int = 0):
        """Bloom pass 1 over {key, count} records (include/kc_api.h kc_bloom_records_device)."""
        self._chk(self.lib.kc_bloom_records_device(self._ctx, ctypes.c_void_p(rec_ptr), n_records,
                                                   ctypes.c_void_p(stream or None)), "kc_bloom_records_device")

    def count_records_device(self, rec_ptr: int, n_records: int, stream: int = 0):
        """The counting pass over {key, count} records behind the gate (kc_count_records_device)."""
        self._chk(self.lib.kc_count_records_device(self._ctx, ctypes.c_void_p(rec_ptr), n_records,
                                                   ctypes.c_void_p(stream or None)), "kc_count_records_device")

    def insert_counts_device(self, rec_ptr: int, n_records: int, stream: int = 0):
        self._chk(self.lib.kc_insert_counts_device(self._ctx, ctypes.c_void_p(rec_ptr), n_records,
                                                   ctypes.c_void_p(stream or None)), "kc_insert_counts_device")

    def insert_counts_runs_device(self, rec_ptr: int, group_counts: Sequence[int], stream: int = 0):
        """Records in per-sender groups, each in kc_route_table_device order."""
        arr = (ctypes.c_uint64 * len(group_counts))(*group_counts)
        self._chk(self.lib.kc_insert_counts_runs_device(self._ctx, ctypes.c_void_p(rec_ptr), arr, len(group_counts),
                                                        ctypes.c_void_p(stream or None)),
                  "kc_insert_counts_runs_device")

    def key_words(self) -> int:
        return self.lib.kc_key_words(self._ctx)

    # -- Bloom filter test hooks (kc_bloom_info / kc_bloom_read / kc_bloom_write)
    def bloom_info(self) -> dict:
        nw, bits = ctypes.c_uint64(), ctypes.c_uint64()
        nh, ng, lay = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._chk(self.lib.kc_bloom_info(self._ctx, ctypes.byref(nw), ctypes.byref(bits), ctypes.byref(nh),
                                         ctypes.byref(ng), ctypes.byref(lay)), "kc_bloom_info")
        return {"words": nw.value, "bits": bits.value, "nh": nh.value, "nh_gate": ng.value,
                "layout": "blocked" if lay.value else "reference"}

    def bloom_read(self) -> np.ndarray:
        n = self.bloom_info()["words"]
        a = np.zeros(n, dtype=np.uint32)
        self._chk(self.lib.kc_bloom_read(self._ctx, a.ctypes.data, n), "kc_bloom_read")
        return a

    def bloom_write(self, words: np.ndarray):
        a = np.ascontiguousarray(words, dtype=np.uint32)
        self._chk(self.lib.kc_bloom_write(self._ctx, a.ctypes.data, a.size), "kc_bloom_write")

    # -- sharded Bloom filter (kc_bloom_get/merge/set_device, kc_bloom_estimate)
    def bloom_get_device(self, dst_ptr: int, first_word: int, n_words: int, stream: int = 0):
        self._chk(self.lib.kc_bloom_get_device(self._ctx, ctypes.c_void_p(dst_ptr), first_word, n_words,
                                               ctypes.c_void_p(stream or None)), "kc_bloom_get_device")

    def bloom_merge_device(self, parts_ptr: int, nparts: int, n_words: int, out_ptr: int, stream: int = 0):
        self._chk(self.lib.kc_bloom_merge_device(self._ctx, ctypes.c_void_p(parts_ptr), nparts, n_words,
                                                 ctypes.c_void_p(out_ptr), ctypes.c_void_p(stream or None)),
                  "kc_bloom_merge_device")

    def bloom_set_device(self, src_ptr: int, n_words: int, stream: int = 0) -> int:
        """Install a whole filter; returns the new_in_second estimate the table is sized from."""
        n = ctypes.c_uint64()
        self._chk(self.lib.kc_bloom_set_device(self._ctx, ctypes.c_void_p(src_ptr), n_words, ctypes.byref(n),
                                               ctypes.c_void_p(stream or None)), "kc_bloom_set_device")
        return n.value

    def bloom_estimate(self, stream: int = 0) -> int:
        n = ctypes.c_uint64()
        self._chk(self.lib.kc_bloom_estimate(self._ctx, ctypes.byref(n), ctypes.c_void_p(stream or None)),
                  "kc_bloom_estimate")
        return n.value

    def sync(self):
        self._chk(self.lib.kc_sync(self._ctx), "kc_sync")

    def reset(self):
        self._chk(self.lib.kc_reset(self._ctx), "kc_reset")

    def clear_table(self):
        """Empty the table, keep the job's counters (kc_clear_table)."""
        self._chk(self.lib.kc_clear_table(self._ctx), "kc_clear_table")

    def profile(self, enable: bool = True):
        self._chk(self.lib.kc_profile(self._ctx, int(enable)), "kc_profile")

    def timing(self) -> dict:
        t = kc_timing()
        self._chk(self.lib.kc_get_timing(self._ctx, ctypes.byref(t)), "kc_get_timing")
        return {n: getattr(t, n) for n, _ in t._fields_}

    def finish(self) -> dict:
        st = kc_stats()
        self._chk(self.lib.kc_finish(self._ctx, ctypes.byref(st)), "kc_finish")
        return st.as_dict()

    # -- results
    def dump(self) -> np.ndarray:
        """Records as a uint64 array of shape (n, W+1): key words then T(c)."""
        p = ctypes.POINTER(ctypes.c_uint64)()
        n = ctypes.c_uint64()
        self._chk(self.lib.kc_dump(self._ctx, ctypes.byref(p), ctypes.byref(n)), "kc_dump")
        W = self.lib.kc_key_words(self._ctx)
        try:
            if n.value == 0:
                return np.zeros((0, W + 1), dtype=np.uint64)
            arr = np.ctypeslib.as_array(p, shape=(n.value * (W + 1),)).copy()
        finally:
            self.lib.kc_free(p)
        return arr.reshape(-1, W + 1)

    # -- Kaarme's compact representation (kc_compact*)
    def compact(self, load: float = 0.0) -> dict:
        """Build the compact slot words from the counted table; returns kc_compact_info."""
        info = kc_compact_info()
        self._chk(self.lib.kc_compact(self._ctx, load, ctypes.byref(info)), "kc_compact")
        return {n: getattr(info, n) for n, _ in kc_compact_info._fields_}

    def compact_dump(self):
        """(records (n, W+1) as dump(), longest walk, mean walk) reconstructed from the compact words."""
        p = ctypes.POINTER(ctypes.c_uint64)()
        n, mx, mean = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_double()
        self._chk(self.lib.kc_compact_dump(self._ctx, ctypes.byref(p), ctypes.byref(n), ctypes.byref(mx),
                                           ctypes.byref(mean)), "kc_compact_dump")
        W = self.lib.kc_key_words(self._ctx)
        try:
            arr = (np.ctypeslib.as_array(p, shape=(n.value * (W + 1),)).copy() if n.value
                   else np.zeros(0, dtype=np.uint64))
        finally:
            self.lib.kc_free(p)
        return arr.reshape(-1, W + 1), mx.value, mean.value

    def compact_lookup(self, keys: np.ndarray) -> np.ndarray:
        """T(c) of canonical keys (n, W) uint64 (dump's key layout) from the compact words; 0 = absent."""
        k = np.ascontiguousarray(keys, dtype=np.uint64)
        out = np.zeros(k.shape[0], dtype=np.uint32)
        self._chk(self.lib.kc_compact_lookup(self._ctx, k.ctypes.data, k.shape[0], out.ctypes.data),
                  "kc_compact_lookup")
        return out

    # -- queries of the counted table (kc_lookup*, kc_histogram)
    def lookup_device(self, keys_ptr: int, n: int, out_ptr: int, table_keys: bool = False, stream: int = 0):
        """T(c) of n keys in device memory (W uint64 each: dump()'s key layout, either strand, or
        route_device's table keys) into uint32 at out_ptr, 0 = absent; enqueued on `stream`, no wait."""
        self._chk(self.lib.kc_lookup_device(self._ctx, ctypes.c_void_p(keys_ptr or None), n,
                                            KEYS_TABLE if table_keys else KEYS_DUMP, ctypes.c_void_p(out_ptr or None),
                                            ctypes.c_void_p(stream or None)), "kc_lookup_device")

    def lookup(self, keys: np.ndarray, table_keys: bool = False) -> np.ndarray:
        """T(c) of keys (n, W) uint64 (encode_kmers / dump()'s key layout, either strand; or table
        keys); 0 = absent.  The minimum abundance is not applied."""
        W = self.lib.kc_key_words(self._ctx)
        k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, W)
        out = np.zeros(k.shape[0], dtype=np.uint32)
        self._chk(self.lib.kc_lookup(self._ctx, k.ctypes.data, k.shape[0], KEYS_TABLE if table_keys else KEYS_DUMP,
                                     out.ctypes.data), "kc_lookup")
        return out

    def histogram(self, n_bins: int = 16385) -> np.ndarray:
        """The count-of-counts: hist[v] = k-mers with T(c) == v, the last bin holding T(c) >= n_bins - 1."""
        if not 0 <= n_bins < 2 ** 32:
            raise KcError(-1, "kc_histogram: 2 <= n_bins <= 65537")
        out = np.zeros(max(n_bins, 1), dtype=np.uint64)
        self._chk(self.lib.kc_histogram(self._ctx, out.ctypes.data, n_bins), "kc_histogram")
        return out

    # -- sequence queries (kc_text_counts*, kc_seq_stats*)
    def text_counts_device(self, text_ptr: int, n: int, out_ptr: int, stream: int = 0):
        """T(c) of the k-mer starting at each of the n bytes of a text in device memory (A/C/G/T in
        either case are bases, every other byte a break) into n uint32 at out_ptr; NO_KMER where no
        k-mer starts; enqueued on `stream`, no wait."""
        self._chk(self.lib.kc_text_counts_device(self._ctx, ctypes.c_void_p(text_ptr or None), n,
                                                 ctypes.c_void_p(out_ptr or None), ctypes.c_void_p(stream or None)),
                  "kc_text_counts_device")

    def text_counts(self, text: bytes) -> np.ndarray:
        """T(c) of the k-mer starting at every byte of `text` (uint32, NO_KMER where none starts)."""
        text = bytes(text)
        out = np.zeros(len(text), dtype=np.uint32)
        self._chk(self.lib.kc_text_counts(self._ctx, text, len(text), out.ctypes.data), "kc_text_counts")
        return out

    def seq_stats_device(self, text_ptr: int, n_bytes: int, offsets, out_ptr: int, solid_min: int = 1,
                         stream: int = 0):
        """Per-sequence statistics of a text in device memory: sequence i is the bytes
        [offsets[i], offsets[i + 1]) (host offsets, one more than sequences); SEQ_STAT_DTYPE records
        into device memory at out_ptr; enqueued on `stream`."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_seqs = max(len(off) - 1, 0)
        self._chk(self.lib.kc_seq_stats_device(self._ctx, ctypes.c_void_p(text_ptr or None), n_bytes, off.ctypes.data,
                                               n_seqs, solid_min, ctypes.c_void_p(out_ptr or None),
                                               ctypes.c_void_p(stream or None)), "kc_seq_stats_device")

    def seq_stats(self, seqs: Sequence, solid_min: int = 1) -> np.ndarray:
        """Statistics of the k-mer counts of each sequence (str or bytes): a SEQ_STAT_DTYPE array with
        windows, present (T(c) >= 1), solid (T(c) >= solid_min), min, median (lower), max and sum."""
        text, off = pack_sequences(seqs)  # (a sequence's newline is a break: no window holds it)
        out = np.zeros(len(off) - 1, dtype=SEQ_STAT_DTYPE)
        if len(out):
            self._chk(self.lib.kc_seq_stats(self._ctx, text, len(text), off.ctypes.data, len(out), solid_min,
                                            out.ctypes.data), "kc_seq_stats")
        return out

    # -- read correction (kc_correct*)
    def correct_device(self, text_ptr: int, n_bytes: int, offsets, out_ptr: int, solid_min: int = 1,
                       stats_ptr: int = 0, stream: int = 0):
        """Corrects isolated base errors of a text in device memory from the table (the rule:
        include/kc_api.h): sequence i is the bytes [offsets[i], offsets[i + 1]) (host offsets); all
        n_bytes go to out_ptr (out_ptr == text_ptr: in place); CORRECT_STAT_DTYPE records into device
        memory at stats_ptr (0: none); enqueued on `stream`, no wait."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_seqs = max(len(off) - 1, 0)
        self._chk(self.lib.kc_correct_device(self._ctx, ctypes.c_void_p(text_ptr or None), n_bytes, off.ctypes.data,
                                             n_seqs, solid_min, ctypes.c_void_p(out_ptr or None),
                                             ctypes.c_void_p(stats_ptr or None), ctypes.c_void_p(stream or None)),
                  "kc_correct_device")

    def correct(self, seqs: Sequence, solid_min: int = 1) -> Tuple[List[bytes], np.ndarray]:
        """The sequences (str or bytes) with their isolated base errors corrected -- a position all
        of whose k-mers are weaker than solid_min and that exactly one other base makes solid -- and a
        CORRECT_STAT_DTYPE array with candidates, corrected, ambiguous and dropped per sequence."""
        text, off = pack_sequences(seqs)  # (a sequence's newline is a break: no window holds it)
        stats = np.zeros(len(off) - 1, dtype=CORRECT_STAT_DTYPE)
        out = ctypes.create_string_buffer(max(len(text), 1))
        if len(stats):
            self._chk(self.lib.kc_correct(self._ctx, text, len(text), off.ctypes.data, len(stats), solid_min, out,
                                          stats.ctypes.data), "kc_correct")
        fixed = out.raw[:len(text)]
        return [fixed[int(off[i]):int(off[i + 1]) - 1] for i in range(len(stats))], stats

    # -- table algebra (kc_table_op*): this counter is the destination
    def table_op_device(self, a: "KmerCounter", b: "KmerCounter", op: int, a_range=(1, 0), b_range=(1, 0),
                        stats_ptr: int = 0, stream: int = 0):
        """self += op(a, b) on the raw counts (OP_*), all in HBM: a key of a takes part when
        a_range[0] <= T(c) <= a_range[1] (a max of 0: no upper bound), the same for b.  stats_ptr: 40
        bytes of device memory for the kc_op_stats (0: none); enqueued on `stream`, no wait."""
        d = _op_desc(op, a_range, b_range)
        self._chk(self.lib.kc_table_op_device(self._ctx, a._ctx, b._ctx, ctypes.byref(d),
                                              ctypes.c_void_p(stats_ptr or None), ctypes.c_void_p(stream or None)),
                  "kc_table_op_device")

    def table_op(self, a: "KmerCounter", b: "KmerCounter", op: int, a_range=(1, 0), b_range=(1, 0)) -> dict:
        """table_op_device that waits; returns the statistics: a_keys (keys of a in its range), both
        (of those, in b), b_only (UNION ops only), out_keys and out_sum (the records added here)."""
        d, st = _op_desc(op, a_range, b_range), kc_op_stats()
        self._chk(self.lib.kc_table_op(self._ctx, a._ctx, b._ctx, ctypes.byref(d), ctypes.byref(st)), "kc_table_op")
        return st.as_dict()

    # -- the de Bruijn graph of the counted table (kc_neighbors*, kc_graph*)
    def neighbors_device(self, keys_ptr: int, n: int, out_ptr: int, table_keys: bool = False, stream: int = 0):
        """T(c) of the eight neighbours of n keys in device memory (W uint64 each, as lookup_device
        takes them; the strand of a dump-layout key is kept) into 8 uint32 per key at out_ptr:
        [y] = canon(x[1:] + y), [4 + y] = canon(y + x[:-1]); enqueued on `stream`, no wait."""
        self._chk(self.lib.kc_neighbors_device(self._ctx, ctypes.c_void_p(keys_ptr or None), n,
                                               KEYS_TABLE if table_keys else KEYS_DUMP,
                                               ctypes.c_void_p(out_ptr or None), ctypes.c_void_p(stream or None)),
                  "kc_neighbors_device")

    def neighbors(self, keys: np.ndarray, table_keys: bool = False) -> np.ndarray:
        """T(c) of the eight neighbours of keys (n, W) uint64 (encode_kmers' layout, the strand as
        given; or table keys) as an (n, 8) uint32 array: column y the k-mer that follows with base y
        appended, column 4 + y the one that precedes with base y prepended; 0 = absent."""
        W = self.lib.kc_key_words(self._ctx)
        k = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1, W)
        out = np.zeros((k.shape[0], 8), dtype=np.uint32)
        self._chk(self.lib.kc_neighbors(self._ctx, k.ctypes.data, k.shape[0], KEYS_TABLE if table_keys else KEYS_DUMP,
                                        out.ctypes.data), "kc_neighbors")
        return out

    def graph_device(self, min_count: int = 1, max_count: int = 0, records_ptr: int = 0, capacity: int = 0,
                     n_ptr: int = 0, stats_ptr: int = 0, stream: int = 0):
        """The graph of the k-mers with min_count <= T(c) <= max_count (0: no upper bound), all in
        device memory: W + 1 uint64 per node at records_ptr (0: none; at most `capacity` are
        written), the number of nodes at n_ptr and the 80-byte kc_graph_stats at stats_ptr (0: none);
        enqueued on `stream`, no wait."""
        self._chk(self.lib.kc_graph_device(self._ctx, min_count, max_count, ctypes.c_void_p(records_ptr or None),
                                           capacity, ctypes.c_void_p(n_ptr or None), ctypes.c_void_p(stats_ptr or None),
                                           ctypes.c_void_p(stream or None)), "kc_graph_device")

    def graph(self, min_count: int = 1, max_count: int = 0) -> Tuple[np.ndarray, dict]:
        """(records, statistics) of the de Bruijn graph whose nodes are the k-mers with min_count <=
        T(c) <= max_count: records (n, W + 1) uint64, the key words as dump() and then T(c) | flags <<
        32 (flags: GRAPH_*); the statistics as graph_stats()."""
        p = ctypes.POINTER(ctypes.c_uint64)()
        n, st = ctypes.c_uint64(), kc_graph_stats()
        self._chk(self.lib.kc_graph(self._ctx, min_count, max_count, ctypes.byref(p), ctypes.byref(n), ctypes.byref(st)),
                  "kc_graph")
        W = self.lib.kc_key_words(self._ctx)
        try:
            arr = (np.ctypeslib.as_array(p, shape=(n.value * (W + 1),)).copy() if n.value
                   else np.zeros(0, dtype=np.uint64))
        finally:
            self.lib.kc_free(p)
        return arr.reshape(-1, W + 1), st.as_dict()

    def graph_stats(self, min_count: int = 1, max_count: int = 0) -> dict:
        """The graph's statistics without its records: nodes, edge_ends, link_ends, isolated,
        palindromes, side_degree[0..4] and open_unitigs (the non-circular unitigs)."""
        st = kc_graph_stats()
        self._chk(self.lib.kc_graph(self._ctx, min_count, max_count, None, None, ctypes.byref(st)), "kc_graph")
        return st.as_dict()

    # -- the unitigs of that graph (kc_unitigs*)
    def unitigs_device(self, min_count: int = 1, max_count: int = 0, unitigs_ptr: int = 0, cap_unitigs: int = 0,
                       bases_ptr: int = 0, cap_bases: int = 0, stats_ptr: int = 0, stream: int = 0):
        """The unitigs of the graph whose nodes are the k-mers with min_count <= T(c) <= max_count,
        all in device memory: a 32-byte kc_unitig {offset, n_nodes, count_sum, flags} per unitig at
        unitigs_ptr (record i only when i < cap_unitigs), its n_nodes + k - 1 ASCII bases at
        bases_ptr + offset (only when they end at or before cap_bases) and the 40-byte
        kc_unitig_stats, always the full totals, at stats_ptr; each pointer may be 0.  Enqueued on
        `stream`, no wait."""
        self._chk(self.lib.kc_unitigs_device(self._ctx, min_count, max_count, ctypes.c_void_p(unitigs_ptr or None),
                                             cap_unitigs, ctypes.c_void_p(bases_ptr or None), cap_bases,
                                             ctypes.c_void_p(stats_ptr or None), ctypes.c_void_p(stream or None)),
                  "kc_unitigs_device")

    def unitigs(self, min_count: int = 1, max_count: int = 0) -> Tuple[np.ndarray, np.ndarray, dict]:
        """(records, bases, statistics): records (n, 4) uint64 {offset, n_nodes, count_sum, flags} in
        an unspecified order, bases a uint8 array of ASCII ACGT that holds unitig i's n_nodes + k - 1
        bases from records[i, 0] on (unitig_strings cuts them out), the statistics as
        unitig_stats()."""
        pr, pb, st = ctypes.POINTER(kc_unitig)(), ctypes.POINTER(ctypes.c_uint8)(), kc_unitig_stats()
        self._chk(self.lib.kc_unitigs(self._ctx, min_count, max_count, ctypes.byref(pr), ctypes.byref(pb),
                                      ctypes.byref(st)), "kc_unitigs")
        try:
            recs = (np.ctypeslib.as_array(ctypes.cast(pr, ctypes.POINTER(ctypes.c_uint64)), shape=(st.unitigs * 4,)).copy()
                    if st.unitigs else np.zeros(0, dtype=np.uint64))
            bases = np.ctypeslib.as_array(pb, shape=(st.bases,)).copy() if st.bases else np.zeros(0, dtype=np.uint8)
        finally:
            self.lib.kc_free(pr)
            self.lib.kc_free(pb)
        return recs.reshape(-1, 4), bases, st.as_dict()

    def unitig_stats(self, min_count: int = 1, max_count: int = 0) -> dict:
        """The unitigs' totals without records or bases: unitigs, circular, nodes, bases (= nodes +
        (k - 1) * unitigs) and max_nodes (the longest unitig)."""
        st = kc_unitig_stats()
        self._chk(self.lib.kc_unitigs(self._ctx, min_count, max_count, None, None, ctypes.byref(st)), "kc_unitigs")
        return st.as_dict()

    # -- the compacted graph: the unitigs and the edges between them (kc_unitig_graph*)
    def unitig_graph_device(self, min_count: int = 1, max_count: int = 0, unitigs_ptr: int = 0, cap_unitigs: int = 0,
                            bases_ptr: int = 0, cap_bases: int = 0, edges_ptr: int = 0, cap_edges: int = 0,
                            stats_ptr: int = 0, stream: int = 0):
        """unitigs_device plus the edges between the unitigs, all in device memory: a 16-byte
        kc_unitig_edge {from, to, flags, 0} per edge at edges_ptr (edge j only when j < cap_edges;
        from and to are record indices of this call's unitig records, flags EDGE_FROM_REV |
        EDGE_TO_REV) and the 64-byte kc_cdbg_stats, always the full totals, at stats_ptr; each
        pointer may be 0.  Enqueued on `stream`, no wait."""
        self._chk(self.lib.kc_unitig_graph_device(self._ctx, min_count, max_count, ctypes.c_void_p(unitigs_ptr or None),
                                                  cap_unitigs, ctypes.c_void_p(bases_ptr or None), cap_bases,
                                                  ctypes.c_void_p(edges_ptr or None), cap_edges,
                                                  ctypes.c_void_p(stats_ptr or None), ctypes.c_void_p(stream or None)),
                  "kc_unitig_graph_device")

    def unitig_graph(self, min_count: int = 1, max_count: int = 0) -> Tuple[np.ndarray, np.ndarray, np.ndarray, dict]:
        """(records, bases, edges, statistics): records and bases as unitigs() gives them, edges an
        EDGE_DTYPE array in an unspecified order whose from and to index the records, the statistics
        as unitig_graph_stats().  gfa_lines writes them as GFA."""
        pr, pb, pe = ctypes.POINTER(kc_unitig)(), ctypes.POINTER(ctypes.c_uint8)(), ctypes.POINTER(kc_unitig_edge)()
        st = kc_cdbg_stats()
        self._chk(self.lib.kc_unitig_graph(self._ctx, min_count, max_count, ctypes.byref(pr), ctypes.byref(pb),
                                           ctypes.byref(pe), ctypes.byref(st)), "kc_unitig_graph")
        try:
            recs = (np.ctypeslib.as_array(ctypes.cast(pr, ctypes.POINTER(ctypes.c_uint64)), shape=(st.unitigs * 4,)).copy()
                    if st.unitigs else np.zeros(0, dtype=np.uint64))
            bases = np.ctypeslib.as_array(pb, shape=(st.bases,)).copy() if st.bases else np.zeros(0, dtype=np.uint8)
            edges = (np.ctypeslib.as_array(ctypes.cast(pe, ctypes.POINTER(ctypes.c_uint32)), shape=(st.edges * 4,)).copy()
                     if st.edges else np.zeros(0, dtype=np.uint32))
        finally:
            self.lib.kc_free(pr)
            self.lib.kc_free(pb)
            self.lib.kc_free(pe)
        return recs.reshape(-1, 4), bases, edges.view(EDGE_DTYPE), st.as_dict()

    def unitig_graph_stats(self, min_count: int = 1, max_count: int = 0) -> dict:
        """The compacted graph's totals without records, bases or edges: unitig_stats()' five, edges
        (edge records) and dead_ends (unitig ends without any edge)."""
        st = kc_cdbg_stats()
        self._chk(self.lib.kc_unitig_graph(self._ctx, min_count, max_count, None, None, None, ctypes.byref(st)),
                  "kc_unitig_graph")
        return st.as_dict()

    # -- read paths through the compacted graph (kc_read_paths*)
    def read_paths_device(self, text_ptr: int, n_bytes: int, offsets, min_count: int = 1, max_count: int = 0,
                          unitigs_ptr: int = 0, cap_unitigs: int = 0, bases_ptr: int = 0, cap_bases: int = 0,
                          edges_ptr: int = 0, cap_edges: int = 0, cdbg_stats_ptr: int = 0, runs_ptr: int = 0,
                          cap_runs: int = 0, seq_ptr: int = 0, path_stats_ptr: int = 0, stream: int = 0):
        """unitig_graph_device plus the paths of a text in device memory through that graph: sequence
        i is the bytes [offsets[i], offsets[i + 1]) (host offsets); a 32-byte kc_path_run per run at
        runs_ptr in text order (run j only when j < cap_runs), a kc_path_seq per sequence at seq_ptr
        and the 64-byte kc_path_stats, always the full totals, at path_stats_ptr; each pointer may be
        0.  Enqueued on `stream`, no wait."""
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        n_seqs = max(len(off) - 1, 0)
        v = lambda x: ctypes.c_void_p(x or None)
        self._chk(self.lib.kc_read_paths_device(self._ctx, min_count, max_count, v(unitigs_ptr), cap_unitigs, v(bases_ptr),
                                                cap_bases, v(edges_ptr), cap_edges, v(cdbg_stats_ptr), v(text_ptr), n_bytes,
                                                off.ctypes.data if len(off) else None, n_seqs, v(runs_ptr), cap_runs,
                                                v(seq_ptr), v(path_stats_ptr), v(stream)), "kc_read_paths_device")

    def read_paths(self, seqs: Sequence, min_count: int = 1, max_count: int = 0):
        """(records, bases, edges, cdbg statistics, runs, per-sequence array, path statistics): the
        compacted graph as unitig_graph() gives it and, through the same call's records, the paths of
        the sequences (str or bytes): a RUN_DTYPE array in text order (text_pos counts in
        pack_sequences' text), a PATH_SEQ_DTYPE array and the totals.  gaf_lines writes them as GAF."""
        text, off = pack_sequences(seqs)
        n_seqs = len(off) - 1
        pr, pb, pe = ctypes.POINTER(kc_unitig)(), ctypes.POINTER(ctypes.c_uint8)(), ctypes.POINTER(kc_unitig_edge)()
        pu, ps = ctypes.POINTER(kc_path_run)(), ctypes.POINTER(kc_path_seq)()
        st, pst = kc_cdbg_stats(), kc_path_stats()
        self._chk(self.lib.kc_read_paths(self._ctx, min_count, max_count, ctypes.byref(pr), ctypes.byref(pb),
                                         ctypes.byref(pe), ctypes.byref(st), text, len(text), off.ctypes.data, n_seqs,
                                         ctypes.byref(pu), ctypes.byref(ps), ctypes.byref(pst)), "kc_read_paths")
        try:
            recs = (np.ctypeslib.as_array(ctypes.cast(pr, ctypes.POINTER(ctypes.c_uint64)), shape=(st.unitigs * 4,)).copy()
                    if st.unitigs else np.zeros(0, dtype=np.uint64))
            bases = np.ctypeslib.as_array(pb, shape=(st.bases,)).copy() if st.bases else np.zeros(0, dtype=np.uint8)
            edges = (np.ctypeslib.as_array(ctypes.cast(pe, ctypes.POINTER(ctypes.c_uint32)), shape=(st.edges * 4,)).copy()
                     if st.edges else np.zeros(0, dtype=np.uint32))
            runs = (np.ctypeslib.as_array(ctypes.cast(pu, ctypes.POINTER(ctypes.c_uint32)), shape=(pst.runs * 8,)).copy()
                    if pst.runs else np.zeros(0, dtype=np.uint32))
            per = (np.ctypeslib.as_array(ctypes.cast(ps, ctypes.POINTER(ctypes.c_uint32)), shape=(n_seqs * 8,)).copy()
                   if n_seqs else np.zeros(0, dtype=np.uint32))
        finally:
            for p_ in (pr, pb, pe, pu, ps):
                self.lib.kc_free(p_)
        return (recs.reshape(-1, 4), bases, edges.view(EDGE_DTYPE), st.as_dict(), runs.view(RUN_DTYPE),
                per.view(PATH_SEQ_DTYPE), pst.as_dict())

    def read_path_stats(self, seqs: Sequence, min_count: int = 1, max_count: int = 0) -> dict:
        """The path totals of the sequences without records or runs: seqs, windows, located, runs,
        chains and threaded (sequences whose windows form one chain)."""
        text, off = pack_sequences(seqs)
        pst = kc_path_stats()
        self._chk(self.lib.kc_read_paths(self._ctx, min_count, max_count, None, None, None, None, text, len(text),
                                         off.ctypes.data, len(off) - 1, None, None, ctypes.byref(pst)), "kc_read_paths")
        return pst.as_dict()

    # -- graph cleaning (kc_clean*): this counter is the destination
    def clean_device(self, src: "KmerCounter", min_count: int = 1, max_count: int = 0, tip_max_nodes: int = 0,
                     iso_max_nodes: int = 0, max_mean: int = 0, stats_ptr: int = 0, stream: int = 0):
        """self += the graph of src's k-mers with min_count <= T(c) <= max_count without its tips of at
        most tip_max_nodes nodes and its isolated unitigs of at most iso_max_nodes nodes (0: the rule
        is off; k - 1 is customary), none removed whose mean T(c) is above max_mean (0: no guard);
        raw counts, all in HBM.  stats_ptr: 64 bytes of device memory for the kc_clean_stats (0:
        none); enqueued on `stream`, no wait."""
        d = _clean_desc(min_count, max_count, tip_max_nodes, iso_max_nodes, max_mean)
        self._chk(self.lib.kc_clean_device(self._ctx, src._ctx, ctypes.byref(d), ctypes.c_void_p(stats_ptr or None),
                                           ctypes.c_void_p(stream or None)), "kc_clean_device")

    def clean(self, src: "KmerCounter", min_count: int = 1, max_count: int = 0, tip_max_nodes: int = 0,
              iso_max_nodes: int = 0, max_mean: int = 0) -> dict:
        """clean_device that waits; returns the statistics: unitigs and nodes of the range's graph,
        tips, tip_nodes, isolated and isolated_nodes (what was removed), out_keys and out_sum (the
        kept nodes and their raw counts, added here)."""
        d, st = _clean_desc(min_count, max_count, tip_max_nodes, iso_max_nodes, max_mean), kc_clean_stats()
        self._chk(self.lib.kc_clean(self._ctx, src._ctx, ctypes.byref(d), ctypes.byref(st)), "kc_clean")
        return st.as_dict()

    # -- bubble popping (kc_pop_bubbles*): this counter is the destination
    def pop_bubbles_device(self, src: "KmerCounter", min_count: int = 1, max_count: int = 0, max_nodes: int = 0,
                           max_diff: int = 0, max_mean: int = 0, stats_ptr: int = 0, stream: int = 0):
        """self += the graph of src's k-mers with min_count <= T(c) <= max_count without the weaker of
        its parallel unitigs: a branch (both ends of degree 1) of at most max_nodes nodes (0: nothing
        is popped; k is customary) is dropped when a branch between the same two unitig ends, of at
        most max_nodes nodes and at most max_diff nodes longer or shorter, has the higher mean T(c)
        (or the same and the smaller name); none is dropped whose mean T(c) is above max_mean (0: no
        guard); raw counts, all in HBM.  stats_ptr: 64 bytes of device memory for the
        kc_bubble_stats (0: none); enqueued on `stream`, no wait."""
        d = _bubble_desc(min_count, max_count, max_nodes, max_diff, max_mean)
        self._chk(self.lib.kc_pop_bubbles_device(self._ctx, src._ctx, ctypes.byref(d), ctypes.c_void_p(stats_ptr or None),
                                                 ctypes.c_void_p(stream or None)), "kc_pop_bubbles_device")

    def pop_bubbles(self, src: "KmerCounter", min_count: int = 1, max_count: int = 0, max_nodes: int = 0,
                    max_diff: int = 0, max_mean: int = 0) -> dict:
        """pop_bubbles_device that waits; returns the statistics: unitigs and nodes of the range's
        graph, branches, parallel (branches with a parallel branch, whatever the limits), popped and
        popped_nodes (what was dropped), out_keys and out_sum (the kept nodes and their raw counts,
        added here)."""
        d, st = _bubble_desc(min_count, max_count, max_nodes, max_diff, max_mean), kc_bubble_stats()
        self._chk(self.lib.kc_pop_bubbles(self._ctx, src._ctx, ctypes.byref(d), ctypes.byref(st)), "kc_pop_bubbles")
        return st.as_dict()

    # -- weak-link removal (kc_cut_weak*): this counter is the destination
    def cut_weak_device(self, src: "KmerCounter", min_count: int = 1, max_count: int = 0, max_nodes: int = 0,
                        ratio_permille: int = 0, max_mean: int = 0, stats_ptr: int = 0, stream: int = 0):
        """self += the graph of src's k-mers with min_count <= T(c) <= max_count without its short
        interior unitigs of low local coverage: an open, non-palindromic unitig whose ends both have
        an edge, of at most max_nodes nodes (0: nothing is cut; k to 2 k is customary), is dropped
        when its mean T(c) is below ratio_permille / 1000 of the mean T(c) over the nodes of the
        unitigs its edges lead to (0: no relative test; 100 to 200 is customary, and from about 500
        both arms of an even bubble go); none is dropped whose mean T(c) is above max_mean (0: no
        guard); raw counts, all in HBM.  stats_ptr: 64 bytes of device memory for the kc_weak_stats
        (0: none); enqueued on `stream`, no wait."""
        d = _weak_desc(min_count, max_count, max_nodes, ratio_permille, max_mean)
        self._chk(self.lib.kc_cut_weak_device(self._ctx, src._ctx, ctypes.byref(d), ctypes.c_void_p(stats_ptr or None),
                                              ctypes.c_void_p(stream or None)), "kc_cut_weak_device")

    def cut_weak(self, src: "KmerCounter", min_count: int = 1, max_count: int = 0, max_nodes: int = 0,
                 ratio_permille: int = 0, max_mean: int = 0) -> dict:
        """cut_weak_device that waits; returns the statistics: unitigs and nodes of the range's graph,
        interior, weak (interior unitigs that are weak, whatever max_nodes and the guard say), cut and
        cut_nodes (what was dropped), out_keys and out_sum (the kept nodes and their raw counts,
        added here)."""
        d, st = _weak_desc(min_count, max_count, max_nodes, ratio_permille, max_mean), kc_weak_stats()
        self._chk(self.lib.kc_cut_weak(self._ctx, src._ctx, ctypes.byref(d), ctypes.byref(st)), "kc_cut_weak")
        return st.as_dict()

    def compact_read(self, info: dict):
        """(slot words, secondary-array words) as uint64 arrays."""
        W = self.lib.kc_key_words(self._ctx)
        words = np.zeros(info["slots"], dtype=np.uint64)
        second = np.zeros(info["chain_starts"] * W, dtype=np.uint64)
        self._chk(self.lib.kc_compact_read(self._ctx, words.ctypes.data, words.size, second.ctypes.data,
                                           second.size), "kc_compact_read")
        return words, second.reshape(-1, W)

    def lines(self) -> List[str]:
        """Sorted "<KMER> <count>" lines (what sort(kaarme output) yields)."""
        return sorted(f"{s} {c}" for s, c in decode_records(self.dump(), self.cfg.k))

    def write(self, path: str):
        self._chk(self.lib.kc_write(self._ctx, path.encode()), "kc_write")

    def output_digest(self) -> dict:
        """Order-independent digest of the output text (kc_output_digest): lines, sum of T(c), and
        the sum mod 2^64 / XOR of XXH64 over every line (hash_sum / hash_xor as 16 hex digits, the
        format of oracle/kc_digest.c and tests/golden/fullsize.json)."""
        d = kc_digest()
        self._chk(self.lib.kc_output_digest(self._ctx, ctypes.byref(d)), "kc_output_digest")
        return digest_dict(d.lines, d.count_sum, d.hash_sum, d.hash_xor)


def _op_desc(op: int, a_range, b_range) -> kc_op_desc:
    return kc_op_desc(int(op), int(a_range[0]), int(a_range[1]), int(b_range[0]), int(b_range[1]), 0)


def table_compare(a: KmerCounter, b: KmerCounter, a_range=(1, 0), b_range=(1, 0)) -> dict:
    """Compare two counted tables in HBM (kc_table_op without a destination, OP_UNION_SUM): the
    statistics of KmerCounter.table_op plus jaccard = both / (a_keys + b_only) and containment (of a
    in b) = both / a_keys, 0.0 where the denominator is 0.  Nothing is inserted anywhere."""
    d, st = _op_desc(OP_UNION_SUM, a_range, b_range), kc_op_stats()
    a._chk(a.lib.kc_table_op(None, a._ctx, b._ctx, ctypes.byref(d), ctypes.byref(st)), "kc_table_op")
    r = st.as_dict()
    union = r["a_keys"] + r["b_only"]
    r["jaccard"] = r["both"] / union if union else 0.0
    r["containment"] = r["both"] / r["a_keys"] if r["a_keys"] else 0.0
    return r


def _filter_rounds(name, src, rounds, stats_only, into, done, rule) -> Tuple[KmerCounter, List[dict]]:
    """The round driver of clean_rounds, pop_rounds and weak_rounds: stats_only(cur, **rule) sizes the next table,
    into(dst, cur, **rule) fills it, done(statistics) ends the rounds early."""
    if rounds < 1:
        raise ValueError(f"{name}: rounds must be at least 1")
    cur, stats = src, []
    for _ in range(rounds):
        n = stats_only(cur, **rule)["out_keys"]
        dst = KmerCounter(dataclasses.replace(src.cfg, table_slots=n + n // 8 + 4096, bf_enable=False, est_unique=0,
                                              batch_bytes=1 << 20))
        try:
            st = into(dst, cur, **rule)
            dst.finish()
        except Exception:
            dst.close()
            if cur is not src:
                cur.close()
            raise
        if cur is not src:
            cur.close()
        cur = dst
        stats.append(st)
        if done(st):
            break
    return cur, stats


def _clean_desc(min_count, max_count, tip_max_nodes, iso_max_nodes, max_mean) -> kc_clean_desc:
    return kc_clean_desc(int(min_count), int(max_count), int(tip_max_nodes), int(iso_max_nodes), int(max_mean), 0)


def clean_stats(src: KmerCounter, min_count: int = 1, max_count: int = 0, tip_max_nodes: int = 0, iso_max_nodes: int = 0,
                max_mean: int = 0) -> dict:
    """The statistics of KmerCounter.clean without a destination (kc_clean with dst NULL): nothing is
    inserted anywhere, and out_keys sizes a destination."""
    d, st = _clean_desc(min_count, max_count, tip_max_nodes, iso_max_nodes, max_mean), kc_clean_stats()
    src._chk(src.lib.kc_clean(None, src._ctx, ctypes.byref(d), ctypes.byref(st)), "kc_clean")
    return st.as_dict()


def clean_rounds(src: KmerCounter, rounds: int, **rule) -> Tuple[KmerCounter, List[dict]]:
    """Up to `rounds` rounds of graph cleaning, each on the result of the one before (removing tips
    makes longer unitigs and sometimes new tips): (the last round's table, the statistics of every
    round run).  rule: clean()'s keywords, the same in every round.  A round first asks for the
    statistics alone, creates a table of out_keys + out_keys / 8 + 4096 slots (src's k, mode,
    min_abundance and device; no Bloom filter, a 1 MiB stage: it is read, not counted into) and
    cleans into it; the intermediate table before it is closed (src never is).
    The rounds stop early after one that removes nothing.  The caller closes the result."""
    return _filter_rounds("clean_rounds", src, rounds, clean_stats, KmerCounter.clean,
                          lambda st: st["tips"] == 0 and st["isolated"] == 0, rule)


def _bubble_desc(min_count, max_count, max_nodes, max_diff, max_mean) -> kc_bubble_desc:
    return kc_bubble_desc(int(min_count), int(max_count), int(max_nodes), int(max_diff), int(max_mean), 0)


def bubble_stats(src: KmerCounter, min_count: int = 1, max_count: int = 0, max_nodes: int = 0, max_diff: int = 0,
                 max_mean: int = 0) -> dict:
    """The statistics of KmerCounter.pop_bubbles without a destination (kc_pop_bubbles with dst NULL):
    nothing is inserted anywhere, and out_keys sizes a destination."""
    d, st = _bubble_desc(min_count, max_count, max_nodes, max_diff, max_mean), kc_bubble_stats()
    src._chk(src.lib.kc_pop_bubbles(None, src._ctx, ctypes.byref(d), ctypes.byref(st)), "kc_pop_bubbles")
    return st.as_dict()


def pop_rounds(src: KmerCounter, rounds: int, **rule) -> Tuple[KmerCounter, List[dict]]:
    """Up to `rounds` rounds of bubble popping, each on the result of the one before (popping joins
    unitigs, and a longer unitig can be an arm of a wider bubble): (the last round's table, the
    statistics of every round run).  rule: pop_bubbles()'s keywords, the same in every round.  A
    round first asks for the statistics alone, creates a table of out_keys + out_keys / 8 + 4096
    slots (src's k, mode, min_abundance and device; no Bloom filter, a 1 MiB stage: it is read, not
    counted into) and pops into it; the intermediate table before it is closed (src never is).
    The rounds stop early after one that pops nothing.  The caller closes the result."""
    return _filter_rounds("pop_rounds", src, rounds, bubble_stats, KmerCounter.pop_bubbles,
                          lambda st: st["popped"] == 0, rule)


def _weak_desc(min_count, max_count, max_nodes, ratio_permille, max_mean) -> kc_weak_desc:
    return kc_weak_desc(int(min_count), int(max_count), int(max_nodes), int(ratio_permille), int(max_mean), 0)


def weak_stats(src: KmerCounter, min_count: int = 1, max_count: int = 0, max_nodes: int = 0, ratio_permille: int = 0,
               max_mean: int = 0) -> dict:
    """The statistics of KmerCounter.cut_weak without a destination (kc_cut_weak with dst NULL):
    nothing is inserted anywhere, and out_keys sizes a destination."""
    d, st = _weak_desc(min_count, max_count, max_nodes, ratio_permille, max_mean), kc_weak_stats()
    src._chk(src.lib.kc_cut_weak(None, src._ctx, ctypes.byref(d), ctypes.byref(st)), "kc_cut_weak")
    return st.as_dict()


def weak_rounds(src: KmerCounter, rounds: int, **rule) -> Tuple[KmerCounter, List[dict]]:
    """Up to `rounds` rounds of weak-link removal, each on the result of the one before (cutting joins
    unitigs, which changes the neighbours of what is left): (the last round's table, the statistics
    of every round run).  rule: cut_weak()'s keywords, the same in every round.  A round first asks
    for the statistics alone, creates a table of out_keys + out_keys / 8 + 4096 slots (src's k, mode,
    min_abundance and device; no Bloom filter, a 1 MiB stage: it is read, not counted into) and cuts
    into it; the intermediate table before it is closed (src never is).
    The rounds stop early after one that cuts nothing.  The caller closes the result."""
    return _filter_rounds("weak_rounds", src, rounds, weak_stats, KmerCounter.cut_weak, lambda st: st["cut"] == 0, rule)


def digest_dict(lines: int, count_sum: int, hash_sum: int, hash_xor: int) -> dict:
    return {"lines": int(lines), "count_sum": int(count_sum), "hash_sum": f"{int(hash_sum) & (2**64 - 1):016x}",
            "hash_xor": f"{int(hash_xor) & (2**64 - 1):016x}"}


def combine_digests(parts: Iterable[dict]) -> dict:
    """The digest of the union of disjoint line sets (e.g. the owners of a sharded job)."""
    n = c = s = x = 0
    for d in parts:
        n += d["lines"]
        c += d["count_sum"]
        s += int(d["hash_sum"], 16)
        x ^= int(d["hash_xor"], 16)
    return digest_dict(n, c, s, x)


def same_digest(a: dict, b: dict) -> bool:
    return all(a[key] == b[key] for key in ("lines", "count_sum", "hash_sum", "hash_xor"))


def count_file(path: str, k: int, mode: int = 2, min_abundance: int = 2, table_slots: int = 1 << 20,
               bf_enable: bool = False, est_unique: int = 0, fpr: float = 0.01, chunk_size: int = 0,
               batch_bytes: int = 0, device: int = 0) -> Tuple[KmerCounter, dict]:
    """The parse_input_* functor chain (main.cpp:427-543) on one device, host chunks."""
    with open(path, "rb") as f:
        image = f.read()
    fmt = detect_format(path, image[0] if image else 0)
    chunks = plan_chunks(image, k, fmt, chunk_size)
    if not batch_bytes:  # a small input gets a stage of its own size (one batch, little pinned memory)
        staged = 4096 + sum((ln + 4095) // 4096 * 4096 for _, ln, _ in chunks)
        batch_bytes = staged if staged <= (256 << 20) else 0
    kc = KmerCounter(Config(k=k, mode=mode, table_slots=table_slots, bf_enable=bf_enable,
                            est_unique=est_unique, fpr=fpr, min_abundance=min_abundance,
                            batch_bytes=batch_bytes, device=device))
    mv = memoryview(image)
    if bf_enable:
        for off, ln, bh in chunks:
            kc.bloom_chunk(bytes(mv[off:off + ln]), fmt, bool(bh))
        kc.bloom_finalize()
    for off, ln, bh in chunks:
        kc.count_chunk(bytes(mv[off:off + ln]), fmt, bool(bh))
    stats = kc.finish()
    return kc, stats
