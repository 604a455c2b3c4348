"""GPU probe: time of the compacted graph (kc_unitig_graph_device) beside kc_unitigs_device with records
and bases on the same table and range as the yardstick: what the edges between the unitigs add to the
unitigs alone.  Writes one JSON record (--out).

  c2      the bench generator's reads (150 bp, 10 M reads = C2, -m 2 -s 200000000), counted at each
          k of --ks (31 and 127: one- and four-word keys).
  forms   kc_unitig_graph_device with records, bases and edges; with records and bases but no edge
          buffer (the edges are counted, none is probed); statistics only; each at the ranges (1, 0)
          and (2, 0).  The device form has no host wait and sizes its node ids by the table's slots.
  report  ms (median, min, max), the ratio to kc_unitigs_device, the kc_cdbg_stats totals and the
          scratch bytes (5 per slot + 144 per id).

HIP events around each call, the functions taking turns in one process, median (min, max) of --reps
after --warmup.

Run it on the GPU box under a time limit, e.g.
  timeout -k 10 500 python canonical-k-mer-hash-table_amd/tools/cdbg_time.py --out kc_out/cdbg_time.json
"""
import argparse
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
ap.add_argument("--ks", default="31,127")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default="")
args = ap.parse_args()
G = 50_000_000

lib = ka.load_library()
stream = torch.cuda.current_stream().cuda_stream
FIELDS = ("unitigs", "circular", "nodes", "bases", "max_nodes", "edges", "dead_ends", "reserved")


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
    return [{"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "all_ms": t} for t in ts]


def measure(kc, K):
    st = kc.finish()
    out = {"key_words": ka.words_for_k(K), "distinct": st["distinct"], "table_slots": st["table_slots"],
           "scratch_bytes_device_form": 5 * st["table_slots"] + 144 * st["table_slots"]}
    cstats = torch.zeros(8, dtype=torch.int64, device="cuda")
    ustats = torch.zeros(5, dtype=torch.int64, device="cuda")
    for lo in (1, 2):
        kc.unitig_graph_device(lo, 0, stats_ptr=cstats.data_ptr(), stream=stream)
        torch.cuda.synchronize()
        tot = dict(zip(FIELDS, cstats.cpu().tolist()))
        nu, nb, ne = tot["unitigs"], tot["bases"], tot["edges"]
        recs = torch.empty(max(1, nu) * 4, dtype=torch.int64, device="cuda")
        bases = torch.empty(max(1, nb), dtype=torch.uint8, device="cuda")
        edges = torch.empty(max(1, ne) * 4, dtype=torch.int32, device="cuda")
        fns = (lambda: kc.unitigs_device(lo, 0, recs.data_ptr(), nu, bases.data_ptr(), nb, ustats.data_ptr(), stream),
               lambda: kc.unitig_graph_device(lo, 0, recs.data_ptr(), nu, bases.data_ptr(), nb, edges.data_ptr(), ne,
                                              cstats.data_ptr(), stream),
               lambda: kc.unitig_graph_device(lo, 0, recs.data_ptr(), nu, bases.data_ptr(), nb, 0, 0, cstats.data_ptr(),
                                              stream),
               lambda: kc.unitig_graph_device(lo, 0, stats_ptr=cstats.data_ptr(), stream=stream))
        names = ("unitigs_with_bases", "cdbg_with_edges", "cdbg_records_no_edges", "cdbg_stats_only")
        rec = dict(zip(names, interleaved_ms(fns)))
        torch.cuda.synchronize()
        assert dict(zip(FIELDS, cstats.cpu().tolist())) == tot and ustats.cpu().tolist() == cstats.cpu().tolist()[:5]
        for name in names[1:]:
            rec[name]["over_unitigs_with_bases"] = rec[name]["ms"] / rec["unitigs_with_bases"]["ms"]
        rec["stats"] = {f: tot[f] for f in FIELDS[:7]}
        out["range_%d_0" % lo] = rec
        del recs, bases, edges
    return out


result = {"lib": os.environ.get("KC_LIB", "lib/libkc.so"), "reads": args.reads, "genome": G, "slots": args.slots, "by_k": {}}
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

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
