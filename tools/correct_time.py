"""GPU probe: time of the read correction (kc_correct_device) on a C2-sized table -- the bench
generator's 10 M x 150 bp reads, k = 31, 51 and 127 -- beside kc_seq_stats_device on the same text in
the same process.  Writes one JSON record (--out).

  text       the first 250 MiB of the input image (the slice seq_probe.py uses), one sequence per
             FASTA record (a record's header and newline are break bytes of its sequence).
  yardstick  kc_seq_stats_device(solid_min) on that text: pack, per-position counts, reduction.
  correct    kc_correct_device(solid_min) out of place with the per-sequence counters: pack, counts,
             mark, try, apply.  The two take turns, HIP events around each call, median (min, max)
             of --reps after --warmup.
  uncounted  the same two calls on --uncounted-mib of reads of another genome (seed and genome
             differ): no k-mer of theirs is in the table, so every base position is a candidate and
             every alternative fails at its first round -- the worst case of the try kernel.

--only-correct runs nothing but --reps correction calls of one k (the run to put under
rocprofv3 --kernel-trace --stats).

Run it on the GPU box under a time limit, e.g.
  timeout -k 10 500 python tools/correct_time.py --out kc_out/correct_time.json
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
ap.add_argument("--uncounted-mib", type=int, default=16)
ap.add_argument("--ks", default="31,51,127")
ap.add_argument("--solid-min", type=int, default=2)
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--only-correct", action="store_true")
ap.add_argument("--out", default="")
args = ap.parse_args()
L, G = 150, 50_000_000

lib = ka.load_library()
stream = torch.cuda.current_stream().cuda_stream


def synth(seed, genome, reads):
    n = lib.kc_synth_bytes(0, reads, L, 0)
    img = torch.empty(n, dtype=torch.uint8, device="cuda")
    assert lib.kc_synth_device(img.data_ptr(), 0, reads, seed, genome, L, 0, 0.001, 0.0, 0) == 0
    torch.cuda.synchronize()
    return img, n


def records(img, n_text):
    """one sequence per record: the offsets of the '>' bytes, and the text's end"""
    starts = (img[:n_text] == ord(">")).nonzero().flatten().cpu().numpy().astype(np.uint64)
    return np.append(starts, np.uint64(n_text))


def interleaved_ms(fns, reps, warmup):
    """per function: median (min, max) of the timed repetitions, HIP events; the functions take turns"""
    ts = [[] for _ in fns]
    for i in range(warmup + reps):
        for j, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if i >= warmup:
                ts[j].append(a.elapsed_time(b))
    return [{"ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "reps": len(t)} for t in ts]


def pair(kc, text, n_text, off, reps, warmup):
    """the yardstick and the correction on one text -> (seq_stats record, correct record)"""
    n_seqs = len(off) - 1
    sstats = torch.zeros(n_seqs * 32, dtype=torch.uint8, device="cuda")
    cstats = torch.zeros(n_seqs * 16, dtype=torch.uint8, device="cuda")
    out = torch.empty(n_text, dtype=torch.uint8, device="cuda")

    def yard():
        kc.seq_stats_device(text.data_ptr(), n_text, off, sstats.data_ptr(), solid_min=args.solid_min, stream=stream)

    def fix():
        kc.correct_device(text.data_ptr(), n_text, off, out.data_ptr(), args.solid_min, cstats.data_ptr(), stream)

    if args.only_correct:
        (c,) = interleaved_ms([fix], reps, 1)
        y = None
    else:
        y, c = interleaved_ms([yard, fix], reps, warmup)
        y["windows"] = int(sstats.cpu().numpy().view(ka.SEQ_STAT_DTYPE)["windows"].sum())
    got = cstats.cpu().numpy().view(ka.CORRECT_STAT_DTYPE)
    c["sequences"] = n_seqs
    for f in got.dtype.names:
        c[f] = int(got[f].sum())
    c["candidates_per_sequence"] = c["candidates"] / max(1, n_seqs)
    c["sequences_with_candidates"] = int((got["candidates"] > 0).sum())
    c["bytes_changed"] = int((out != text[:n_text]).sum())
    if y:
        c["over_seq_stats"] = c["ms"] / y["ms"]
    return y, c


img, nbytes = synth(42, G, args.reads)
other, obytes = synth(7, G + 1_000_003, max(1, (args.uncounted_mib << 20) // (L + 12)))
result = {"lib": os.environ.get("KC_LIB", "lib/libkc.so"), "reads": args.reads, "read_len": L, "genome": G,
          "solid_min": args.solid_min, "k": {}}
for k in [int(x) for x in args.ks.split(",")]:
    chunks = ka.plan_chunks_device(img.data_ptr(), nbytes, k, ka.FMT_FASTA)
    sl = [c for c in chunks if c[0] + c[1] <= (args.slice_mib << 20)]
    n_text = sl[-1][0] + sl[-1][1]  # the slice: whole chunks, so whole records
    rec = {"slice_bytes": n_text}
    with ka.KmerCounter(ka.Config(k=k, mode=2, table_slots=200_000_000, min_abundance=1)) as kc:
        kc.count_device(img.data_ptr(), chunks, ka.FMT_FASTA, stream)
        st = kc.finish()
        rec["distinct"], rec["table_slots"] = st["distinct"], st["table_slots"]
        y, c = pair(kc, img, n_text, records(img, n_text), args.reps, args.warmup)
        rec["seq_stats"], rec["correct"] = y, c
        if not args.only_correct:
            y, c = pair(kc, other, obytes, records(other, obytes), 3, 1)
            rec["uncounted_bytes"], rec["uncounted_seq_stats"], rec["uncounted_correct"] = obytes, y, c
    result["k"][str(k)] = rec
    print(f"k={k}: {json.dumps(rec)}", flush=True)

if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
