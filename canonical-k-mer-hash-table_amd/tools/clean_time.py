"""GPU probe: time of graph cleaning (kc_clean_device) beside the two calls it is made of, on the same
table, as the yardsticks: kc_unitig_graph_device statistics-only (the ranking and the heads) and
kc_table_op_device KC_OP_INTERSECT_LEFT of the table with itself into a fresh destination of the
table's size (a sweep, a probe and the inserts).  Writes one JSON record (--out).

  c2      the bench generator's reads (150 bp, 10 M reads = C2, -m 2 -s 200000000), counted at each
          k of --ks (31 and 127: one- and four-word keys).
  forms   kc_clean_device at the range (2, 0) with tip_max_nodes = iso_max_nodes = k - 1: statistics
          only; into a destination of out_keys + out_keys / 8 + 4096 slots (the size clean_rounds and
          the CLI give it); into a destination of the table's size (the yardstick's).  Every
          destination is emptied and zero-filled before the timed call, outside the events.
  report  ms (median, min, max), the ratio to the sum of the two yardsticks, the kc_clean_stats
          totals of one round and of three rounds (clean_rounds, wall time), and the scratch bytes
          (5 per slot + 141 per id; the device form sizes its ids by the table's slots).

HIP events around each call, the functions taking turns in one process, median (min, max) of --reps
after --warmup.

Run it on the GPU box under a time limit, e.g.
  timeout -k 10 500 python canonical-k-mer-hash-table_amd/tools/clean_time.py --out kc_out/clean_time.json
"""
import argparse
import json
import os
import statistics
import sys
import time

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
LO, HI = 2, 0

lib = ka.load_library()
stream = torch.cuda.current_stream().cuda_stream
FIELDS = ("unitigs", "nodes", "tips", "tip_nodes", "isolated", "isolated_nodes", "out_keys", "out_sum")


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


def measure(kc, K):
    st = kc.finish()
    rule = dict(tip_max_nodes=K - 1, iso_max_nodes=K - 1)
    out = {"key_words": ka.words_for_k(K), "distinct": st["distinct"], "table_slots": st["table_slots"],
           "range": [LO, HI], "rule": rule, "scratch_bytes_device_form": 5 * st["table_slots"] + 141 * st["table_slots"]}
    one = ka.clean_stats(kc, LO, HI, **rule)
    out["stats_one_round"] = one
    n = one["out_keys"]
    cfg = dict(k=K, mode=2, min_abundance=1, batch_bytes=1 << 20)
    dstats = torch.zeros(8, dtype=torch.int64, device="cuda")
    gstats = torch.zeros(8, dtype=torch.int64, device="cuda")
    ostats = torch.zeros(5, dtype=torch.int64, device="cuda")
    with ka.KmerCounter(ka.Config(table_slots=n + n // 8 + 4096, **cfg)) as sized, \
            ka.KmerCounter(ka.Config(table_slots=args.slots, **cfg)) as big:
        out["sized_dst_slots"], out["same_size_dst_slots"] = sized.finish()["table_slots"], big.finish()["table_slots"]
        clean = dict(min_count=LO, max_count=HI, stats_ptr=dstats.data_ptr(), stream=stream, **rule)
        fns = ((None, lambda: kc.unitig_graph_device(LO, HI, stats_ptr=gstats.data_ptr(), stream=stream)),
               (emptied(big), lambda: big.table_op_device(kc, kc, ka.OP_INTERSECT_LEFT, stats_ptr=ostats.data_ptr(),
                                                          stream=stream)),
               (emptied(big), lambda: big.table_op_device(kc, kc, ka.OP_INTERSECT_LEFT, a_range=(LO, HI),
                                                          stats_ptr=ostats.data_ptr(), stream=stream)),
               (None, lambda: lib.kc_clean_device(None, kc._ctx, ka.kc_clean_desc(LO, HI, K - 1, K - 1, 0, 0),
                                                  dstats.data_ptr(), stream)),
               (emptied(sized), lambda: sized.clean_device(kc, **clean)),
               (emptied(big), lambda: big.clean_device(kc, **clean)))
        names = ("cdbg_stats_only", "intersect_left_self", "intersect_left_self_range_2_0", "clean_stats_only",
                 "clean_into_sized_dst", "clean_into_same_size_dst")
        rec = dict(zip(names, interleaved_ms(fns)))
        torch.cuda.synchronize()
        assert dict(zip(FIELDS, dstats.cpu().tolist())) == one, (dstats.cpu().tolist(), one)
        assert big.finish()["inserted"] == one["out_sum"]
        yard = rec["cdbg_stats_only"]["ms"] + rec["intersect_left_self"]["ms"]
        out["yardsticks_sum_ms"] = yard
        for name in names[3:]:
            rec[name]["over_yardsticks_sum"] = rec[name]["ms"] / yard
        rec["clean_stats_only"]["over_cdbg_stats_only"] = rec["clean_stats_only"]["ms"] / rec["cdbg_stats_only"]["ms"]
        out.update(rec)
    t0 = time.perf_counter()
    last, rounds = ka.clean_rounds(kc, 3, min_count=LO, max_count=HI, **rule)
    out["three_rounds_wall_s"] = time.perf_counter() - t0
    last.close()
    out["stats_three_rounds"] = rounds
    assert rounds[0] == one
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
