"""GPU probe: time of the unitig layer (kc_unitigs_device) beside kc_graph_device statistics-only on
the same table and range -- the two sweeps of the table a unitig call cannot avoid -- as the
yardstick.  Writes one JSON record (--out).

  c2      the bench generator's reads (150 bp, 10 M reads = C2, -m 2 -s 200000000), counted at each
          k of --ks (31, 51, 127: one-, two- and four-word keys).
  long    error-free 10 kbp reads (--long-reads of them, C5's generator) at k = 127: long chains, so
          the ranking has 15 - 20 live rounds.
  forms   kc_unitigs_device with bases and records, with records only, statistics only; each at the
          ranges (1, 0) and (2, 0).  The device form has no host wait and sizes its node ids by the
          table's slots.
  report  ms (median, min, max), the ratio to the yardstick, unitigs / circular / nodes / bases /
          longest, the scratch bytes (5 per slot + 140 per id), and the jump rounds that did work:
          the API does not return them, so they are derived from the statistics -- round r of the
          first ranking runs while a state is farther than 2^r from its end, that is 1 +
          floor(log2(longest - 1)) rounds, or every round up to log2(2 nodes) when there is a circle.

HIP events around each call, the functions taking turns in one process, median (min, max) of --reps
after --warmup.  The split between the kernels comes from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats -- python .../unitig_time.py --ks 31 --reps 2 --warmup 1 --long-reads 0).

Run it on the GPU box under a time limit, e.g.
  timeout -k 10 500 python canonical-k-mer-hash-table_amd/tools/unitig_time.py --out kc_out/unitig_time.json
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import kaarme_amd as ka  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--slots", type=int, default=200_000_000)
ap.add_argument("--ks", default="31,51,127")
ap.add_argument("--long-reads", type=int, default=20_000)
ap.add_argument("--long-slots", type=int, default=200_000_000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default="")
args = ap.parse_args()
G = 50_000_000

lib = ka.load_library()
stream = torch.cuda.current_stream().cuda_stream
FIELDS = ("unitigs", "circular", "nodes", "bases", "max_nodes")


def interleaved_ms(fns):
    """per function: median (min, max) of the timed repetitions, HIP events; the functions take turns"""
    ts = [[] for _ in fns]
    for i in range(args.warmup + args.reps):
        for j, fn in enumerate(fns):
            a_ev, b_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a_ev.record()
            fn()
            b_ev.record()
            b_ev.synchronize()
            if i >= args.warmup:
                ts[j].append(a_ev.elapsed_time(b_ev))
    return [{"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "reps": len(t)} for t in ts]


def rounds_worked(st):
    if not st["nodes"]:
        return 0
    if st["circular"]:
        return int(math.floor(math.log2(2 * st["nodes"]))) + 1
    return 1 + (int(math.floor(math.log2(st["max_nodes"] - 1))) if st["max_nodes"] > 1 else 0)


def measure(kc, K):
    st = kc.finish()
    out = {"key_words": ka.words_for_k(K), "distinct": st["distinct"], "table_slots": st["table_slots"],
           "scratch_bytes_device_form": 5 * st["table_slots"] + 140 * st["table_slots"],
           "rounds_enqueued_per_ranking": int(math.ceil(math.log2(2 * st["table_slots"]))) + 1}
    dstats = torch.zeros(5, dtype=torch.int64, device="cuda")
    gstats = torch.zeros(10, dtype=torch.int64, device="cuda")
    for lo in (1, 2):
        kc.unitigs_device(lo, 0, 0, 0, 0, 0, dstats.data_ptr(), stream)
        torch.cuda.synchronize()
        tot = dict(zip(FIELDS, dstats.cpu().tolist()))
        recs = torch.empty(max(1, tot["unitigs"]) * 4, dtype=torch.int64, device="cuda")
        bases = torch.empty(max(1, tot["bases"]), dtype=torch.uint8, device="cuda")
        fns = (lambda: kc.graph_device(lo, 0, 0, 0, 0, gstats.data_ptr(), stream),
               lambda: kc.unitigs_device(lo, 0, recs.data_ptr(), tot["unitigs"], bases.data_ptr(), tot["bases"],
                                         dstats.data_ptr(), stream),
               lambda: kc.unitigs_device(lo, 0, recs.data_ptr(), tot["unitigs"], 0, 0, dstats.data_ptr(), stream),
               lambda: kc.unitigs_device(lo, 0, 0, 0, 0, 0, dstats.data_ptr(), stream))
        names = ("graph_stats_only", "unitigs_with_bases", "unitigs_records_only", "unitigs_stats_only")
        rec = dict(zip(names, interleaved_ms(fns)))
        torch.cuda.synchronize()
        assert dict(zip(FIELDS, dstats.cpu().tolist())) == tot and int(gstats[0].item()) == tot["nodes"]
        for name in names[1:]:
            rec[name]["over_graph_stats_only"] = rec[name]["ms"] / rec["graph_stats_only"]["ms"]
        rec["stats"] = tot
        rec["rounds_worked_first_ranking"] = rounds_worked(tot)
        rec["exact_id_scratch_bytes"] = 5 * st["table_slots"] + 140 * tot["nodes"]
        out["range_%d_0" % lo] = rec
        del recs, bases
    return out


result = {"lib": os.environ.get("KC_LIB", "lib/libkc.so"), "reads": args.reads, "genome": G, "slots": args.slots,
          "by_k": {}, "long": None}
if args.reads:
    L = 150
    n_img = lib.kc_synth_bytes(0, args.reads, L, 0)
    img = torch.empty(n_img, dtype=torch.uint8, device="cuda")
    assert lib.kc_synth_device(img.data_ptr(), 0, args.reads, 42, G, L, 0, 0.001, 0.0, 0) == 0
    torch.cuda.synchronize()
    for K in (int(x) for x in args.ks.split(",")):
        chunks = ka.plan_chunks_device(img.data_ptr(), n_img, K, ka.FMT_FASTA)
        with ka.KmerCounter(ka.Config(k=K, mode=2, table_slots=args.slots, min_abundance=1)) as kc:
            kc.count_device(img.data_ptr(), chunks, ka.FMT_FASTA, stream)
            result["by_k"][str(K)] = measure(kc, K)
        print(f"k={K}: {json.dumps(result['by_k'][str(K)])}", flush=True)
    del img
if args.long_reads:
    K, L = 127, 10_000
    n_img = lib.kc_synth_bytes(0, args.long_reads, L, 0)
    img = torch.empty(n_img, dtype=torch.uint8, device="cuda")
    assert lib.kc_synth_device(img.data_ptr(), 0, args.long_reads, 43, G, L, 0, 0.0, 0.0, 0) == 0
    torch.cuda.synchronize()
    chunks = ka.plan_chunks_device(img.data_ptr(), n_img, K, ka.FMT_FASTA)
    with ka.KmerCounter(ka.Config(k=K, mode=2, table_slots=args.long_slots, min_abundance=1)) as kc:
        kc.count_device(img.data_ptr(), chunks, ka.FMT_FASTA, stream)
        result["long"] = dict(measure(kc, K), reads=args.long_reads, read_len=L, k=K)
    print(f"long: {json.dumps(result['long'])}", flush=True)

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
