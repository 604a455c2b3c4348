"""GPU probe: time of weak-link removal (kc_cut_weak_device) beside its yardsticks on the same table,
all measured in the same run: kc_clean_device (rules k - 1) into a destination of the table's size,
kc_unitig_graph_device with the edge buffer and kc_unitigs_device statistics-only.  Writes one JSON
record (--out).

  c2      the bench generator's reads (150 bp, 10 M reads = C2, -m 2 -s 200000000), counted at each
          k of --ks (31 and 127: one- and four-word keys).
  forms   at the ranges (1, 0) and (2, 0): kc_cut_weak_device with max_nodes = k, ratio_permille =
          200, statistics only and into a destination of the table's size; the three yardsticks.
          Every destination is emptied and zero-filled before the timed call, outside the events.
  report  ms (median, min, max); what the kernel costs (statistics only, over kc_unitigs_device's
          statistics-only call: the same ranking and heads); the expectation cut <= clean + 2 *
          (unitig graph with edges - unitigs) + the larger of the spreads of cut and clean (the
          pass probes once per edge of an interior unitig's ends, the work of the edges pass, and
          reads two states and T(c) per neighbour besides) and whether it is met; the
          kc_weak_stats and kc_clean_stats totals of one round (the two copies insert different
          numbers of keys); the scratch bytes (5 per slot + 141 per id; the device form sizes its
          ids by the table's slots).

HIP events around each call, the functions taking turns in one process, median (min, max) of --reps
after --warmup.

Run it on the GPU box under a time limit, e.g.
  timeout -k 10 500 python canonical-k-mer-hash-table_amd/tools/weak_time.py --out kc_out/weak_time.json
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
ap.add_argument("--ratio", type=int, default=200)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default="")
args = ap.parse_args()
G = 50_000_000
RANGES = ((1, 0), (2, 0))

lib = ka.load_library()
stream = torch.cuda.current_stream().cuda_stream
FIELDS = ("unitigs", "nodes", "interior", "weak", "cut", "cut_nodes", "out_keys", "out_sum")


def interleaved_ms(fns):
    """per (prepare, call): median (min, max) of the timed repetitions of call, HIP events; prepare runs
    before the events and is waited for; the functions take turns"""
    ts = [[] for _ in fns]
    for i in range(args.warmup + args.reps):
        for j, (prep, fn) in enumerate(fns):
            if prep:
                prep()
                torch.cuda.synchronize()
            a_ev, b_ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a_ev.record()
            fn()
            b_ev.record()
            b_ev.synchronize()
            if i >= args.warmup:
                ts[j].append(a_ev.elapsed_time(b_ev))
    return [{"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "all_ms": t} for t in ts]


def emptied(dst):
    """dst empty and zero-filled (kc_reset defers the fill to the next use; kc_finish is one)"""
    def prep():
        dst.reset()
        dst.finish()
    return prep


def measure(kc, big, K, lo, hi):
    rule = dict(max_nodes=K, ratio_permille=args.ratio)
    one = ka.weak_stats(kc, lo, hi, **rule)
    out = {"range": [lo, hi], "rule": rule, "stats_one_round": one,
           "clean_stats_one_round": ka.clean_stats(kc, lo, hi, tip_max_nodes=K - 1, iso_max_nodes=K - 1)}
    n_edges = kc.unitig_graph_stats(lo, hi)["edges"]
    edges = torch.empty(max(1, n_edges) * 16, dtype=torch.uint8, device="cuda")
    wstats = torch.zeros(8, dtype=torch.int64, device="cuda")
    cstats = torch.zeros(8, dtype=torch.int64, device="cuda")
    gstats = torch.zeros(8, dtype=torch.int64, device="cuda")
    cut = dict(min_count=lo, max_count=hi, stats_ptr=wstats.data_ptr(), stream=stream, **rule)
    fns = ((None, lambda: kc.unitigs_device(lo, hi, stats_ptr=gstats.data_ptr(), stream=stream)),
           (None, lambda: kc.unitig_graph_device(lo, hi, edges_ptr=edges.data_ptr(), cap_edges=n_edges,
                                                 stats_ptr=gstats.data_ptr(), stream=stream)),
           (emptied(big), lambda: big.clean_device(kc, lo, hi, tip_max_nodes=K - 1, iso_max_nodes=K - 1,
                                                   stats_ptr=cstats.data_ptr(), stream=stream)),
           (None, lambda: lib.kc_cut_weak_device(None, kc._ctx, ka.kc_weak_desc(lo, hi, K, args.ratio, 0, 0), wstats.data_ptr(),
                                                 stream)),
           (emptied(big), lambda: big.cut_weak_device(kc, **cut)))
    names = ("unitigs_stats_only", "cdbg_with_edges", "clean_into_same_size_dst", "cut_stats_only", "cut_into_same_size_dst")
    rec = dict(zip(names, interleaved_ms(fns)))
    torch.cuda.synchronize()
    assert dict(zip(FIELDS, wstats.cpu().tolist())) == one, (wstats.cpu().tolist(), one)
    assert big.finish()["inserted"] == one["out_sum"]
    out["edges"] = n_edges
    cut_ms, clean = rec["cut_into_same_size_dst"], rec["clean_into_same_size_dst"]
    spread = max(cut_ms["max_ms"] - cut_ms["min_ms"], clean["max_ms"] - clean["min_ms"])
    edges_pass = rec["cdbg_with_edges"]["ms"] - rec["unitigs_stats_only"]["ms"]
    bound = clean["ms"] + 2 * edges_pass + spread
    out["expectation"] = {"bound_ms": bound, "edges_pass_ms": edges_pass, "larger_spread_ms": spread, "cut_ms": cut_ms["ms"],
                          "met": cut_ms["ms"] <= bound, "over_bound_ms": cut_ms["ms"] - bound}
    rec["cut_stats_only"]["over_unitigs_stats_only_ms"] = rec["cut_stats_only"]["ms"] - rec["unitigs_stats_only"]["ms"]
    rec["cut_into_same_size_dst"]["over_clean"] = cut_ms["ms"] / clean["ms"]
    out.update(rec)
    return out


result = {"lib": os.environ.get("KC_LIB", "lib/libkc.so"), "reads": args.reads, "genome": G, "slots": args.slots, "by_k": {}}
L = 150
n_img = lib.kc_synth_bytes(0, args.reads, L, 0)
img = torch.empty(n_img, dtype=torch.uint8, device="cuda")
assert lib.kc_synth_device(img.data_ptr(), 0, args.reads, 42, G, L, 0, 0.001, 0.0, 0) == 0
torch.cuda.synchronize()
for K in (int(x) for x in args.ks.split(",")):
    chunks = ka.plan_chunks_device(img.data_ptr(), n_img, K, ka.FMT_FASTA)
    cfg = dict(k=K, mode=2, min_abundance=1)
    with ka.KmerCounter(ka.Config(table_slots=args.slots, **cfg)) as kc, \
            ka.KmerCounter(ka.Config(table_slots=args.slots, batch_bytes=1 << 20, **cfg)) as big:
        kc.count_device(img.data_ptr(), chunks, ka.FMT_FASTA, stream)
        st = kc.finish()
        rec = {"key_words": ka.words_for_k(K), "distinct": st["distinct"], "table_slots": st["table_slots"],
               "same_size_dst_slots": big.finish()["table_slots"],
               "scratch_bytes_device_form": 5 * st["table_slots"] + 141 * st["table_slots"], "by_range": {}}
        for lo, hi in RANGES:
            rec["by_range"][f"{lo},{hi}"] = measure(kc, big, K, lo, hi)
            print(f"k={K} range=({lo}, {hi}): {json.dumps(rec['by_range'][f'{lo},{hi}'])}", flush=True)
        result["by_k"][str(K)] = rec

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
