"""GPU probe: rates of the sequence queries (kc_text_counts_device, kc_seq_stats_device) on a
C2-sized table -- the bench generator's 10 M x 150 bp reads, k = 31, and the same reads at k = 51
and k = 127.  Writes one JSON record (--out).

  counts    kc_text_counts_device over the first 250 MiB of the input image (the slice
            lookup_probe.py routes; header bytes are breaks, so its windows are the reads' windows),
            and beside it, interleaved in the same process, the two calls that answered the same
            question before: kc_route_device with one shard on a second context, then
            kc_lookup_device(KC_KEYS_TABLE).  HIP events, median of --reps after --warmup; windows/s
            and the bucket reads n x 128 B as a fraction of 8 TB/s.  The two paths' answers are
            compared as multisets (the routed order carries no positions).
  stats     kc_seq_stats_device over the same slice, one sequence per FASTA record, and the share
            of its time that is not the per-position pass (reduction and offsets).

Run it on the GPU box under a time limit, e.g.
  timeout -k 10 500 python tools/seq_probe.py --out kc_out/seq_probe.json
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "canonical-k-mer-hash-table_amd"))
import kaarme_amd as ka  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--slice-mib", type=int, default=250)
ap.add_argument("--ks", default="31,51,127")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()
L, G, HBM = 150, 50_000_000, 8e12

lib = ka.load_library()
nbytes = lib.kc_synth_bytes(0, args.reads, L, 0)
img = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
assert lib.kc_synth_device(img.data_ptr(), 0, args.reads, 42, G, L, 0, 0.001, 0.0, 0) == 0
torch.cuda.synchronize()
stream = torch.cuda.current_stream().cuda_stream


def interleaved_ms(fns):
    """per function: median (min, max) of the timed repetitions, HIP events; the functions take turns"""
    ts = [[] for _ in fns]
    for i in range(args.warmup + args.reps):
        for j, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= args.warmup:
                ts[j].append(a.elapsed_time(b))
    return [{"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "reps": len(t)} for t in ts]


def rate(rec, n):
    rec["windows"] = n
    rec["windows_per_s"] = n / (rec["ms"] * 1e-3)
    rec["bucket_read_fraction_of_8TBps"] = n * 128 / (rec["ms"] * 1e-3) / HBM
    return rec


result = {"lib": os.environ.get("KC_LIB", "lib/libkc.so"), "reads": args.reads, "read_len": L, "genome": G, "k": {}}
for k in [int(x) for x in args.ks.split(",")]:
    W = ka.words_for_k(k)
    chunks = ka.plan_chunks_device(img.data_ptr(), nbytes, k, ka.FMT_FASTA)
    sl = [c for c in chunks if c[0] + c[1] <= (args.slice_mib << 20)]
    n_text = sl[-1][0] + sl[-1][1]  # the slice: whole chunks, so whole records
    rec = {"slice_bytes": n_text}
    with ka.KmerCounter(ka.Config(k=k, mode=2, table_slots=200_000_000, min_abundance=1)) as kc:
        kc.count_device(img.data_ptr(), chunks, ka.FMT_FASTA, stream)
        st = kc.finish()
        rec["distinct"], rec["table_slots"] = st["distinct"], st["table_slots"]
        counts = torch.empty(n_text, dtype=torch.int32, device="cuda")
        used = sum((ln + 4095) // 4096 * 4096 for _, ln, _ in sl)
        cap = used + len(sl)
        with ka.KmerCounter(ka.Config(k=k, mode=2, table_slots=1 << 20, batch_bytes=used + 4096)) as router:
            buf = torch.zeros(cap * W, dtype=torch.int64, device="cuda")
            wout = torch.zeros(cap, dtype=torch.int32, device="cuda")
            routed = []

            def fused():
                kc.text_counts_device(img.data_ptr(), n_text, counts.data_ptr(), stream=stream)

            def two_calls():
                nw = router.route_device(img.data_ptr(), sl, ka.FMT_FASTA, 1, buf.data_ptr(), cap, stream)[0]
                kc.lookup_device(buf.data_ptr(), nw, wout.data_ptr(), table_keys=True, stream=stream)
                routed.append(nw)

            f, t = interleaved_ms([fused, two_calls])
        nw = routed[-1]
        valid = counts != -1  # KC_NO_KMER
        rec["fused_text_counts"] = rate(f, int(valid.sum()))
        rec["route_then_lookup"] = rate(t, nw)
        rec["fused_over_two_calls"] = f["ms"] / t["ms"]
        rec["same_windows"] = int(valid.sum()) == nw
        rec["same_multiset"] = bool(torch.equal(torch.bincount(counts[valid], minlength=16384),
                                                torch.bincount(wout[:nw], minlength=16384)))
        del buf, wout
        # one sequence per record: the offsets of the '>' bytes, and the slice's end
        starts = (img[:n_text] == ord(">")).nonzero().flatten().cpu().numpy().astype(np.uint64)
        off = np.append(starts, np.uint64(n_text))
        stats = torch.zeros((len(off) - 1) * 32, dtype=torch.uint8, device="cuda")
        (s,) = interleaved_ms([lambda: kc.seq_stats_device(img.data_ptr(), n_text, off, stats.data_ptr(), solid_min=2,
                                                           stream=stream)])
        (c,) = interleaved_ms([fused])
        got = stats.cpu().numpy().view(ka.SEQ_STAT_DTYPE)
        s["sequences"] = len(got)
        s["windows"] = int(got["windows"].sum())
        s["windows_per_s"] = s["windows"] / (s["ms"] * 1e-3)
        s["share_not_in_the_counts_pass"] = max(0.0, 1 - c["ms"] / s["ms"])
        s["sum_matches_counts"] = int(got["sum"].sum()) == int(counts[valid].sum(dtype=torch.int64))
        rec["seq_stats"] = s
        del counts, stats
    result["k"][str(k)] = rec
    print(f"k={k}: {json.dumps(rec)}", flush=True)

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
