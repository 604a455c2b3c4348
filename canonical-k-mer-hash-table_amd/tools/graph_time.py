"""GPU probe: time of the de Bruijn graph layer (kc_graph_device, kc_neighbors_device) on a C2-sized
table, beside kc_lookup_device on the same table as the yardstick.  Writes one JSON record (--out).

  table     the bench generator's reads (150 bp, 10 M reads = C2, -m 2 -s 200000000), counted at each
            k of --ks (31: 86.5 M k-mers; 51 and 127: two- and four-word keys).
  graph     kc_graph_device with records (capacity = the nodes) at the ranges (1, 0) and (2, 0), and
            statistics only at (1, 0): both sweeps (k_graph_edges: eight probes per node;
            k_graph_links: one probe per side of degree 1, the statistics, the records).
  neighbors kc_neighbors_device on --keys canonical keys taken from the graph's records (all
            present), eight probes per key.
  lookup    kc_lookup_device on the same keys: one probe per key.  The keys come in table order, so
            these lookups stream through the table; a k-mer's neighbours hash anywhere, so
            lookup_shuffled -- the same keys in a random order, every probe its own 128-byte line
            of HBM -- is the yardstick of the graph's probes.  The edge pass is eight probes per
            node: graph_over_8_lookups = graph ms / (8 x nodes x lookup ms per key) says how far
            the two sweeps are from eight lookups' time per node, against either order.

HIP events around each call, the functions taking turns in one process, median (min, max) of --reps
after --warmup.  The split between the two graph kernels comes from a kernel trace of this tool
(rocprofv3 --kernel-trace --stats -- python .../graph_time.py --ks 31 --reps 2 --warmup 1).

Run it on the GPU box under a time limit, e.g.
  timeout -k 10 500 python canonical-k-mer-hash-table_amd/tools/graph_time.py --out kc_out/graph_time.json
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
ap.add_argument("--ks", default="31,51,127")
ap.add_argument("--keys", type=int, default=10_000_000)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--out", default="")
args = ap.parse_args()
L, G = 150, 50_000_000

lib = ka.load_library()
stream = torch.cuda.current_stream().cuda_stream
FIELDS = ("nodes", "edge_ends", "link_ends", "isolated", "palindromes", "side_degree_0", "side_degree_1", "side_degree_2",
          "side_degree_3", "side_degree_4")


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


n_img = lib.kc_synth_bytes(0, args.reads, L, 0)
img = torch.empty(n_img, dtype=torch.uint8, device="cuda")
assert lib.kc_synth_device(img.data_ptr(), 0, args.reads, 42, G, L, 0, 0.001, 0.0, 0) == 0
torch.cuda.synchronize()

result = {"lib": os.environ.get("KC_LIB", "lib/libkc.so"), "reads": args.reads, "read_len": L, "genome": G,
          "slots": args.slots, "keys": args.keys, "by_k": {}}
for K in (int(x) for x in args.ks.split(",")):
    W = ka.words_for_k(K)
    chunks = ka.plan_chunks_device(img.data_ptr(), n_img, K, ka.FMT_FASTA)
    with ka.KmerCounter(ka.Config(k=K, mode=2, table_slots=args.slots, min_abundance=1)) as kc:
        kc.count_device(img.data_ptr(), chunks, ka.FMT_FASTA, stream)
        st = kc.finish()
        cap = st["distinct"]
        recs = torch.empty(cap * (W + 1), dtype=torch.int64, device="cuda")
        dn = torch.zeros(1, dtype=torch.int64, device="cuda")
        dstats = torch.zeros(10, dtype=torch.int64, device="cuda")

        def graph(lo, hi, with_records=True):
            return lambda: kc.graph_device(lo, hi, recs.data_ptr() if with_records else 0, cap, dn.data_ptr(),
                                           dstats.data_ptr(), stream)

        graph(1, 0)()
        torch.cuda.synchronize()
        assert int(dn.item()) == cap
        n_keys = min(args.keys, cap)
        keys = recs.view(-1, W + 1)[:n_keys, :W].contiguous()
        nb = torch.empty(n_keys * 8, dtype=torch.int32, device="cuda")
        cnt = torch.empty(n_keys, dtype=torch.int32, device="cuda")
        shuffled = keys[torch.randperm(n_keys, device="cuda")].contiguous()
        names = ("graph_1_0", "graph_2_0", "graph_1_0_stats_only", "neighbors", "lookup", "lookup_shuffled")
        fns = (graph(1, 0), graph(2, 0), graph(1, 0, False),
               lambda: kc.neighbors_device(keys.data_ptr(), n_keys, nb.data_ptr(), stream=stream),
               lambda: kc.lookup_device(keys.data_ptr(), n_keys, cnt.data_ptr(), stream=stream),
               lambda: kc.lookup_device(shuffled.data_ptr(), n_keys, cnt.data_ptr(), stream=stream))
        out = {"key_words": W, "distinct": cap, "table_slots": st["table_slots"],
               "table_bytes": st["table_slots"] // (16 // (W + 1)) * 128}
        for name, rec, fn in zip(names, interleaved_ms(fns), fns):
            if name.startswith("graph"):
                fn()
                torch.cuda.synchronize()
                rec["stats"] = dict(zip(FIELDS, dstats.cpu().tolist()))
            out[name] = rec
        assert int((cnt > 0).sum().item()) == n_keys  # the keys are the table's own
        out["lookups_per_s"] = n_keys / (out["lookup"]["ms"] * 1e-3)
        out["shuffled_lookups_per_s"] = n_keys / (out["lookup_shuffled"]["ms"] * 1e-3)
        out["neighbor_keys_per_s"] = n_keys / (out["neighbors"]["ms"] * 1e-3)
        out["neighbors_over_8_lookups"] = out["neighbors"]["ms"] / (8 * out["lookup"]["ms"])
        out["neighbors_over_8_shuffled_lookups"] = out["neighbors"]["ms"] / (8 * out["lookup_shuffled"]["ms"])
        for name in names[:3]:
            nodes = out[name]["stats"]["nodes"]
            out[name]["nodes_per_s"] = nodes / (out[name]["ms"] * 1e-3)
            for y in ("lookup", "lookup_shuffled"):
                out[name]["graph_over_8_%ss" % y] = out[name]["ms"] / (8 * nodes * out[y]["ms"] / n_keys) if nodes else None
        result["by_k"][str(K)] = out
        print(f"k={K}: {json.dumps(out)}", flush=True)
        del recs, keys, shuffled, nb, cnt

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
