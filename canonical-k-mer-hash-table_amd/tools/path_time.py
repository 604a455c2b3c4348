"""GPU probe: time of the read paths (kc_read_paths_device) beside the two calls it cannot be cheaper
than on the same table and text, kc_unitig_graph_device plus kc_text_counts_device.  Writes one JSON
record (--out).

  c2      the bench generator's reads (150 bp, 10 M reads = C2, -m 2 -s 200000000), counted at each
          k of --ks (31 and 127: one- and four-word keys).
  text    the first --text-mb MiB of the counted FASTA image, cut back to a line end; every line is a
          sequence of its own (a header line holds no window at these k).
  forms   kc_read_paths_device with everything (records, bases, edges, runs, per-sequence records);
          with records and runs only; statistics only; each at the ranges (1, 0) and (2, 0).
  report  ms (median, min, max), windows per second of the text, the ratio to the sum of
          kc_unitig_graph_device (everything) and kc_text_counts_device, and the kc_path_stats totals.

HIP events around each call, the functions taking turns in one process, median (min, max) of --reps
after --warmup.

Run it on the GPU box under a time limit, e.g.
  timeout -k 10 500 python canonical-k-mer-hash-table_amd/tools/path_time.py --out kc_out/path_time.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import kaarme_amd as ka  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--slots", type=int, default=200_000_000)
ap.add_argument("--ks", default="31,127")
ap.add_argument("--text-mb", type=int, default=64)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default="")
args = ap.parse_args()
G = 50_000_000

lib = ka.load_library()
stream = torch.cuda.current_stream().cuda_stream
CFIELDS = ("unitigs", "circular", "nodes", "bases", "max_nodes", "edges", "dead_ends", "reserved")
PFIELDS = ("seqs", "windows", "located", "runs", "chains", "threaded")


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


def measure(kc, K, text, n_text, off):
    st = kc.finish()
    n_seqs = len(off) - 1
    out = {"key_words": ka.words_for_k(K), "distinct": st["distinct"], "table_slots": st["table_slots"]}
    cstats = torch.zeros(8, dtype=torch.int64, device="cuda")
    pstats = torch.zeros(8, dtype=torch.int64, device="cuda")
    counts = torch.empty(n_text, dtype=torch.int32, device="cuda")
    per = torch.empty(n_seqs * 4, dtype=torch.int64, device="cuda")
    for lo in (1, 2):
        kc.read_paths_device(text, n_text, off, lo, 0, cdbg_stats_ptr=cstats.data_ptr(), path_stats_ptr=pstats.data_ptr(),
                             stream=stream)
        torch.cuda.synchronize()
        tot, ptot = dict(zip(CFIELDS, cstats.cpu().tolist())), dict(zip(PFIELDS, pstats.cpu().tolist()))
        nu, nb, ne, nr = tot["unitigs"], tot["bases"], tot["edges"], ptot["runs"]
        recs = torch.empty(max(1, nu) * 4, dtype=torch.int64, device="cuda")
        bases = torch.empty(max(1, nb), dtype=torch.uint8, device="cuda")
        edges = torch.empty(max(1, ne) * 4, dtype=torch.int32, device="cuda")
        runs = torch.empty(max(1, nr) * 4, dtype=torch.int64, device="cuda")
        fns = (lambda: kc.unitig_graph_device(lo, 0, recs.data_ptr(), nu, bases.data_ptr(), nb, edges.data_ptr(), ne,
                                              cstats.data_ptr(), stream),
               lambda: kc.text_counts_device(text, n_text, counts.data_ptr(), stream),
               lambda: kc.read_paths_device(text, n_text, off, lo, 0, recs.data_ptr(), nu, bases.data_ptr(), nb,
                                            edges.data_ptr(), ne, cstats.data_ptr(), runs.data_ptr(), nr, per.data_ptr(),
                                            pstats.data_ptr(), stream),
               lambda: kc.read_paths_device(text, n_text, off, lo, 0, recs.data_ptr(), nu, runs_ptr=runs.data_ptr(),
                                            cap_runs=nr, path_stats_ptr=pstats.data_ptr(), stream=stream),
               lambda: kc.read_paths_device(text, n_text, off, lo, 0, path_stats_ptr=pstats.data_ptr(), stream=stream))
        names = ("cdbg_with_edges", "text_counts", "paths_everything", "paths_records_and_runs", "paths_stats_only")
        rec = dict(zip(names, interleaved_ms(fns)))
        torch.cuda.synchronize()
        assert dict(zip(PFIELDS, pstats.cpu().tolist())) == ptot
        floor = rec["cdbg_with_edges"]["ms"] + rec["text_counts"]["ms"]
        for name in names[2:]:
            rec[name]["over_cdbg_plus_text_counts"] = rec[name]["ms"] / floor
            rec[name]["text_part_ms"] = rec[name]["ms"] - rec["cdbg_with_edges"]["ms"]
            rec[name]["windows_per_s"] = ptot["windows"] / (rec[name]["ms"] / 1e3)
        rec["text_counts"]["windows_per_s"] = ptot["windows"] / (rec["text_counts"]["ms"] / 1e3)
        rec["cdbg_stats"] = {f: tot[f] for f in CFIELDS[:7]}
        rec["path_stats"] = ptot
        out["range_%d_0" % lo] = rec
        del recs, bases, edges, runs
    return out


result = {"lib": os.environ.get("KC_LIB", "lib/libkc.so"), "reads": args.reads, "genome": G, "slots": args.slots, "by_k": {}}
L = 150
n_img = lib.kc_synth_bytes(0, args.reads, L, 0)
img = torch.empty(n_img, dtype=torch.uint8, device="cuda")
assert lib.kc_synth_device(img.data_ptr(), 0, args.reads, 42, G, L, 0, 0.001, 0.0, 0) == 0
torch.cuda.synchronize()
# the text: the head of the image up to a line end, every line a sequence
head = img[:min(n_img, args.text_mb << 20)].cpu().numpy()
ends = np.flatnonzero(head == 10)
n_text = int(ends[-1]) + 1
off = np.concatenate(([0], ends + 1)).astype(np.uint64)
result["text_bytes"], result["text_seqs"] = n_text, len(off) - 1
for K in (int(x) for x in args.ks.split(",")):
    chunks = ka.plan_chunks_device(img.data_ptr(), n_img, K, ka.FMT_FASTA)
    with ka.KmerCounter(ka.Config(k=K, mode=2, table_slots=args.slots, min_abundance=1)) as kc:
        kc.count_device(img.data_ptr(), chunks, ka.FMT_FASTA, stream)
        result["by_k"][str(K)] = measure(kc, K, img.data_ptr(), n_text, off)
    print(f"k={K}: {json.dumps(result['by_k'][str(K)])}", flush=True)

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
