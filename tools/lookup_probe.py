"""GPU probe: rates of the table queries (kc_lookup_device, kc_lookup, kc_histogram) on a C2-sized
table -- the bench generator's 10 M x 150 bp reads, k = 31 (about 86.5 M k-mers), and the same
reads at k = 51 and k = 127.  Writes one JSON record (--out).

  lookups   kc_lookup_device timed with HIP events (median of --reps after --warmup): N present
            keys in random order, N absent keys, and the routed table keys (kc_route_device on a
            second context) of a 256 MiB slice of the input; lookups/s and the implied random-read
            bandwidth n x 128 B as a fraction of 8 TB/s
  host      kc_lookup of 10 M host keys end to end (copies included), beside kc_compact +
            kc_compact_lookup of the same keys (the only lookup before this one)
  sweep     kc_histogram(16385) beside kc_output_digest: two sweeps of the same table

KC_LIB picks the build (tools/build_variant.sh: UNITS=query ... -DKC_QUERY_TPK is the
thread-per-key form of the one- and two-word lookups); --what compact,digest runs only what a build
without the query entry points has (with KC_PKG = the directory holding that build's kaarme_amd
package).  Run it on the GPU box under a time limit, e.g.
  timeout -k 10 400 python tools/lookup_probe.py --out kc_out/lookup_probe.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

# KC_PKG: import kaarme_amd from another tree (an older commit's package beside its library in KC_LIB)
sys.path.insert(0, os.environ.get("KC_PKG") or os.path.join(os.path.dirname(__file__), "..", "canonical-k-mer-hash-table_amd"))
import kaarme_amd as ka  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reads", type=int, default=10_000_000)
ap.add_argument("--queries", type=int, default=100_000_000)
ap.add_argument("--host-keys", type=int, default=10_000_000)
ap.add_argument("--ks", default="31,51,127")
ap.add_argument("--what", default="lookups,host,compact,histogram,digest")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--out", default="")
args = ap.parse_args()
WHAT = set(args.what.split(","))
L, G, HBM = 150, 50_000_000, 8e12
GATHER = 1 << 22  # rows per torch indexing call

lib = ka.load_library()
nbytes = lib.kc_synth_bytes(0, args.reads, L, 0)
img = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
assert lib.kc_synth_device(img.data_ptr(), 0, args.reads, 42, G, L, 0, 0.001, 0.0, 0) == 0
torch.cuda.synchronize()
stream = torch.cuda.current_stream().cuda_stream


def gpu_ms(fn):
    """median (and min, max) of the timed repetitions, HIP events on the current stream"""
    ts = []
    for i in range(args.warmup + args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        if i >= args.warmup:
            ts.append(a.elapsed_time(b))
    return {"ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": len(ts)}


def wall_ms(fn, reps=5):
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    ts = ts[1:]
    return {"ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "reps": len(ts)}


def rate(rec, n):
    rec["n"] = n
    rec["lookups_per_s"] = n / (rec["ms"] * 1e-3)
    rec["bucket_read_fraction_of_8TBps"] = n * 128 / (rec["ms"] * 1e-3) / HBM
    return rec


result = {"lib": os.environ.get("KC_LIB", "lib/libkc.so"), "reads": args.reads, "read_len": L, "genome": G, "k": {}}
for k in [int(x) for x in args.ks.split(",")]:
    W = ka.words_for_k(k)
    chunks = ka.plan_chunks_device(img.data_ptr(), nbytes, k, ka.FMT_FASTA)
    rec = {}
    with ka.KmerCounter(ka.Config(k=k, mode=2, table_slots=200_000_000, min_abundance=1)) as kc:
        kc.count_device(img.data_ptr(), chunks, ka.FMT_FASTA, stream)
        st = kc.finish()
        rec["distinct"], rec["table_slots"], rec["windows"] = st["distinct"], st["table_slots"], st["windows"]
        rec["table_bytes"] = st["table_slots"] // (16 // (W + 1)) * 128
        full = kc.dump()
        host_keys = np.ascontiguousarray(full[:args.host_keys, :W])
        host_counts = full[:args.host_keys, W].astype(np.uint32)
        if "lookups" in WHAT:
            n = args.queries
            dkeys = torch.from_numpy(full[:, :W].astype(np.int64, copy=True)).cuda()
            dcounts = torch.from_numpy(full[:, W].astype(np.int32)).cuda()
            idx = torch.randint(0, dkeys.shape[0], (n,), device="cuda")
            q = torch.empty((n, W), dtype=torch.int64, device="cuda")
            want = torch.empty(n, dtype=torch.int32, device="cuda")
            for i in range(0, n, GATHER):  # (one indexing call of 2^26 two-word rows came back wrong)
                q[i:i + GATHER] = dkeys[idx[i:i + GATHER]]
                want[i:i + GATHER] = dcounts[idx[i:i + GATHER]]
            out = torch.zeros(n, dtype=torch.int32, device="cuda")
            rec["present"] = rate(gpu_ms(lambda: kc.lookup_device(q.data_ptr(), n, out.data_ptr(), stream=stream)), n)
            rec["present"]["wrong_answers"] = int((out != want).sum())
            rec["present"]["zero_answers"] = int((out == 0).sum())
            del dkeys, dcounts, idx, want
            if k == 31:
                q.copy_(torch.randint(0, 1 << 62, (n, W), device="cuda"))
                rec["absent"] = rate(gpu_ms(lambda: kc.lookup_device(q.data_ptr(), n, out.data_ptr(), stream=stream)), n)
                rec["absent"]["hits"] = int((out != 0).sum())
                # the table keys of the windows of a 256 MiB slice of the input
                sl = [c for c in chunks if c[0] + c[1] <= (256 << 20)]
                used = sum((ln + 4095) // 4096 * 4096 for _, ln, _ in sl)
                cap = used + len(sl)
                with ka.KmerCounter(ka.Config(k=k, mode=2, table_slots=1 << 20, batch_bytes=used + 4096)) as router:
                    buf = torch.zeros(cap * W, dtype=torch.int64, device="cuda")
                    nw = router.route_device(img.data_ptr(), sl, ka.FMT_FASTA, 1, buf.data_ptr(), cap, stream)[0]
                wout = torch.zeros(nw, dtype=torch.int32, device="cuda")
                rec["routed_windows"] = rate(gpu_ms(lambda: kc.lookup_device(buf.data_ptr(), nw, wout.data_ptr(),
                                                                             table_keys=True, stream=stream)), nw)
                rec["routed_windows"]["slice_bytes"] = sum(ln for _, ln, _ in sl)
                rec["routed_windows"]["zero_answers"] = int((wout == 0).sum())
                del buf, wout
            del q, out
        del full
        if "host" in WHAT and k == 31:
            got = []
            rec["kc_lookup_host"] = wall_ms(lambda: got.append(kc.lookup(host_keys)), 3)
            rec["kc_lookup_host"]["n"] = len(host_keys)
            rec["kc_lookup_host"]["all_correct"] = bool((got[-1] == host_counts).all())
        if "histogram" in WHAT:
            rec["kc_histogram_16385"] = wall_ms(lambda: kc.histogram(16385))
            rec["kc_histogram_16385"]["GBps"] = rec["table_bytes"] / rec["kc_histogram_16385"]["ms"] / 1e6
        if "digest" in WHAT:
            rec["kc_output_digest"] = wall_ms(lambda: kc.output_digest())
            rec["kc_output_digest"]["GBps"] = rec["table_bytes"] / rec["kc_output_digest"]["ms"] / 1e6
        if "compact" in WHAT and k == 31:
            got = []

            def compact_path():
                kc.compact()
                got.append(kc.compact_lookup(host_keys))

            rec["kc_compact_plus_lookup_host"] = wall_ms(compact_path, 2)
            rec["kc_compact_plus_lookup_host"]["n"] = len(host_keys)
            rec["kc_compact_plus_lookup_host"]["all_correct"] = bool((got[-1] == host_counts).all())
            t = time.perf_counter()
            kc.compact_lookup(host_keys)
            rec["kc_compact_lookup_host_alone_ms"] = (time.perf_counter() - t) * 1e3
    result["k"][str(k)] = rec
    print(f"k={k}: {json.dumps(rec)}", flush=True)

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
