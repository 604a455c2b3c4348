"""GPU probe: time of the table algebra (kc_table_op_device) on two C2-sized tables, beside the
composition that was the only way to unite two tables before it.  Writes one JSON record (--out).

  tables    a and b: the bench generator's reads (150 bp, k = 31, -m 2 -s 200000000) of one seed
            and one genome, reads [0, N) into a and [N, 2N) into b (N = --reads, 10 M = C2), so the
            two tables share most of their k-mers (the genome's) and differ in the error k-mers.
  fused     INTERSECT_MIN, SUBTRACT and UNION_SUM into a dst of the same -s emptied by
            kc_clear_table before each call (the deferred zero-fill of dst runs inside the timed
            call, for the composition too); and UNION_SUM without a destination (the statistics of
            table_compare: both sweeps and all probes, no insert).
  composed  union-by-sum as it was composed before: kc_route_table_device(1 shard) of a into a
            record buffer in HBM, kc_insert_counts_device of the buffer into dst, the same for b.
            (kc_route_table_device waits on the host for its record count: part of that path.)

HIP events around each call sequence, the functions taking turns in one process, median (min, max)
of --reps after --warmup.  The fused and the composed union must give the same output digest.
Algorithmic bytes: the sweep reads every bucket of a (128 B), every key of a in range reads one
bucket of b and, when it yields a record, one bucket of dst read and two atomics written.

Run it on the GPU box under a time limit, e.g.
  timeout -k 10 500 python canonical-k-mer-hash-table_amd/tools/table_op_time.py --out kc_out/table_op.json
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import kaarme_amd as ka  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--slots", type=int, default=200_000_000)
ap.add_argument("--k", type=int, default=31)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()
L, G, K = 150, 50_000_000, args.k

lib = ka.load_library()
stream = torch.cuda.current_stream().cuda_stream


def counted(first):
    """the table of reads [first, first + N)"""
    n = lib.kc_synth_bytes(first, args.reads, L, 0)
    img = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert lib.kc_synth_device(img.data_ptr(), first, args.reads, 42, G, L, 0, 0.001, 0.0, 0) == 0
    torch.cuda.synchronize()
    chunks = ka.plan_chunks_device(img.data_ptr(), n, K, ka.FMT_FASTA)
    kc = ka.KmerCounter(ka.Config(k=K, mode=2, table_slots=args.slots, min_abundance=1))
    kc.count_device(img.data_ptr(), chunks, ka.FMT_FASTA, stream)
    return kc, kc.finish()


def interleaved_ms(fns):
    """per function: median (min, max) of the timed repetitions, HIP events; the functions take turns"""
    ts = [[] for _ in fns]
    for i in range(args.warmup + args.reps):
        for j, fn in enumerate(fns):
            dst.clear_table()
            a_ev, b_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a_ev.record()
            fn()
            b_ev.record()
            b_ev.synchronize()
            if i >= args.warmup:
                ts[j].append(a_ev.elapsed_time(b_ev))
    return [{"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "reps": len(t)} for t in ts]


a, st_a = counted(0)
b, st_b = counted(args.reads)
dst = ka.KmerCounter(ka.Config(k=K, mode=2, table_slots=args.slots, min_abundance=1))
W = ka.words_for_k(K)
cap = max(st_a["distinct"], st_b["distinct"])
buf = torch.empty(cap * (W + 1), dtype=torch.int64, device="cuda")
dstats = torch.zeros(5, dtype=torch.int64, device="cuda")


def fused(op):
    return lambda: dst.table_op_device(a, b, op, stats_ptr=dstats.data_ptr(), stream=stream)


def stats_only():  # kc_table_op_device(dst = NULL): Jaccard / containment, nothing inserted
    d = ka.kc_op_desc(ka.OP_UNION_SUM, 1, 0, 1, 0, 0)
    rc = lib.kc_table_op_device(None, a._ctx, b._ctx, ctypes.byref(d), ctypes.c_void_p(dstats.data_ptr()),
                                ctypes.c_void_p(stream or None))
    assert rc == 0, rc


def composed():
    for t in (a, b):
        n = t.route_table_device(1, buf.data_ptr(), cap, stream)[0]
        dst.insert_counts_device(buf.data_ptr(), n, stream)


names = ("intersect_min", "subtract", "union_sum", "composed_union_sum", "union_sum_no_dst")
fns = (fused(ka.OP_INTERSECT_MIN), fused(ka.OP_SUBTRACT), fused(ka.OP_UNION_SUM), composed, stats_only)
recs = interleaved_ms(fns)
result = {"lib": os.environ.get("KC_LIB", "lib/libkc.so"), "k": K, "reads_per_table": args.reads, "read_len": L,
          "genome": G, "slots": args.slots, "table_bytes": st_a["table_slots"] // (16 // (W + 1)) * 128,
          "a_distinct": st_a["distinct"], "b_distinct": st_b["distinct"]}
digests = {}
for name, rec, fn in zip(names, recs, fns):
    dst.clear_table()
    fn()
    dst.sync()
    a.sync()
    digests[name] = dst.output_digest()
    rec["result_kmers"] = digests[name]["lines"]
    if name != "composed_union_sum":
        s = dict(zip(("a_keys", "both", "b_only", "out_keys", "out_sum"), dstats.cpu().tolist()))
        rec["stats"] = s
        union = name.startswith("union_sum")
        swept = 2 if union else 1  # tables swept: their buckets read once each
        probes = s["a_keys"] + (st_b["distinct"] if union else 0)
        inserts = 0 if name.endswith("no_dst") else s["out_keys"]
        rec["insert_atomics"] = 2 * inserts  # the slot's CAS claim (or key match) and the count add
        rec["algorithmic_bytes"] = swept * result["table_bytes"] + 128 * probes + (128 + 16) * inserts
        rec["algorithmic_bytes_per_a_key"] = rec["algorithmic_bytes"] / max(1, s["a_keys"])
        rec["fraction_of_8TBps"] = rec["algorithmic_bytes"] / (rec["ms"] * 1e-3) / 8e12
    result[name] = rec
    print(f"{name}: {json.dumps(rec)}", flush=True)
result["union_digests_equal"] = ka.same_digest(digests["union_sum"], digests["composed_union_sum"])
result["fused_over_composed_union"] = result["union_sum"]["ms"] / result["composed_union_sum"]["ms"]
print(json.dumps({"union_digests_equal": result["union_digests_equal"],
                  "fused_over_composed_union": result["fused_over_composed_union"]}), flush=True)
assert result["union_digests_equal"], "the fused and the composed union differ"

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
