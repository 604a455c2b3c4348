"""GPU: the sharded counting path (kc_route_device -> exchange -> kc_insert_keys_device).

One GPU, G emulated ranks: each rank is its own engine (own table) and counts its own
slice of the reads; the all-to-all is emulated in-process by slicing the owner groups.
The per-rank outputs must be disjoint and their union must equal the oracle's count of
the whole input (bit-exact sorted output).  The same ranks over RCCL are what bench.py
runs at N > 1; tests/test_sharded.py covers the collective itself over gloo.
"""
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import GEN, REPO, oracle_count, sorted_digest_file, sorted_digest_lines
import kaarme_amd as ka
from kaarme_amd.sharded import DeviceEngine

pytestmark = pytest.mark.gpu


def _image(path):
    data = open(path, "rb").read()
    return data, torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


@pytest.mark.parametrize("k,mode,G,path", [(31, 2, 2, "direct"), (31, 2, 3, "partitioned"),
                                            (21, 0, 4, "partitioned"), (51, 2, 2, "direct"),
                                            (51, 0, 3, "partitioned"), (95, 1, 2, "partitioned")])
def test_emulated_ranks_union(tmp_path, monkeypatch, k, mode, G, path):
    monkeypatch.setenv("KC_INSERT_PATH", path)
    n_reads = 30000
    per = n_reads // G
    images = []
    for r in range(G):
        fa = tmp_path / f"r{r}.fasta"
        cnt = per if r < G - 1 else n_reads - per * (G - 1)
        subprocess.run([GEN, str(fa), str(n_reads), "150", "200000", "--first", str(r * per), "--count", str(cnt)],
                       check=True)
        images.append(_image(str(fa)))
    whole = tmp_path / "all.fasta"
    with open(whole, "wb") as f:
        for data, _ in images:
            f.write(data)
    engines = [DeviceEngine(ka.Config(k=k, mode=mode, table_slots=400000, min_abundance=1,
                                      batch_bytes=max(len(d) for d, _ in images) * 2 + (1 << 20)))
               for _ in range(G)]
    W = engines[0].W
    stream = torch.cuda.current_stream().cuda_stream
    routed = []
    for r, (data, img) in enumerate(images):
        chunks = ka.plan_chunks(data, k, ka.FMT_FASTA, chunk_size=256 * 1024)
        buf, counts = engines[r].route(img.data_ptr(), chunks, ka.FMT_FASTA, G, stream)
        torch.cuda.synchronize()
        assert sum(counts) == engines[r].kc.finish()["windows"]
        keys = buf[: sum(counts) * W].view(-1, W)
        assert int((keys[:, 0] == 0).sum()) == 0, "table key word 0 is never 0"
        routed.append((buf.clone(), counts))
    for d in range(G):  # emulated all-to-all: rank d receives group d of every source, in rank order
        parts = []
        for buf, counts in routed:
            lo = sum(counts[:d]) * W
            parts.append(buf[lo:lo + counts[d] * W])
        recv = torch.cat(parts)
        n = recv.numel() // W
        engines[d].insert(recv, n, stream)
        torch.cuda.synchronize()
        assert engines[d].kc.finish()["inserted"] == n
    shard_lines = [set(e.kc.lines()) for e in engines]
    kmers = [set(l.rsplit(" ", 1)[0] for l in s) for s in shard_lines]
    for a in range(G):
        for b in range(a + 1, G):
            assert not (kmers[a] & kmers[b]), "a k-mer has two owners"
        assert kmers[a], "empty shard"
    union = set().union(*shard_lines)
    out = tmp_path / "oracle.txt"
    oracle_count(str(whole), k, ["-m", str(mode), "-a", "1"], out)
    assert sorted_digest_lines(union) == sorted_digest_file(out)


@pytest.mark.parametrize("path", ["direct", "partitioned"])
def test_insert_rejects_non_table_keys(monkeypatch, path):
    """Word 0 == 0 marks an empty slot and is never a table key: such keys are skipped
    (no hang, no corrupted slot) and kc_finish reports them."""
    monkeypatch.setenv("KC_INSERT_PATH", path)
    e = DeviceEngine(ka.Config(k=51, mode=0, table_slots=100000, min_abundance=1))
    keys = torch.zeros(2 * 5000, dtype=torch.int64, device="cuda")
    keys[::4] = 12345  # every other key (word 0 of even keys) is a valid table key
    e.insert(keys, 5000, torch.cuda.current_stream().cuda_stream)
    with pytest.raises(ka.KcError, match="not table keys"):
        e.kc.finish()


def _sorted_rows(d):
    return d[np.lexsort(d.T[::-1])]


@pytest.mark.parametrize("call", ["insert_keys_device", "insert_counts_device", "count_records_device"])
@pytest.mark.parametrize("k,name", [(31, "reads.txt"), (51, "edge.fasta")])
def test_inserts_on_a_side_stream(golden_input, k, name, call):
    """The inserts of received keys and records on a caller's stream: the input arrives by a copy on a
    torch.cuda.Stream, the insert is issued on it with nothing waited for in between, and the table
    read through the context afterwards is the one the null-stream insert leaves."""
    path = golden_input(name)
    data, img = _image(path)
    fmt = ka.detect_format(path, data[0])
    chunks = ka.plan_chunks(data, k, fmt)
    W = ka.words_for_k(k)
    cfg = ka.Config(k=k, mode=2, table_slots=1 << 20, min_abundance=1, batch_bytes=len(data) + 4096 * (len(chunks) + 1))
    with ka.KmerCounter(cfg) as src:
        if call == "insert_keys_device":  # the windows' table keys
            item = W
            cap = sum((ln + 4095) // 4096 * 4096 for _, ln, _ in chunks) + len(chunks)
            buf = torch.zeros(cap * item, dtype=torch.int64, device="cuda")
            n = sum(src.route_device(img.data_ptr(), chunks, fmt, 1, buf.data_ptr(), cap))
        else:  # the counted table's {key, count} records
            item = W + 1
            src.count_device(img.data_ptr(), chunks, fmt)
            cap = src.finish()["distinct"]
            buf = torch.zeros(cap * item, dtype=torch.int64, device="cuda")
            n = sum(src.route_table_device(1, buf.data_ptr(), cap))
        torch.cuda.synchronize()
    assert n > 1000
    host = buf[: n * item].cpu().pin_memory()

    def table_after(stream):
        with ka.KmerCounter(cfg) as kc:
            with torch.cuda.stream(stream or torch.cuda.current_stream()):
                dev = torch.empty(n * item, dtype=torch.int64, device="cuda")
                dev.copy_(host, non_blocking=True)
                getattr(kc, call)(dev.data_ptr(), n, stream.cuda_stream if stream else 0)
            return _sorted_rows(kc.dump()), kc.finish()

    want, want_st = table_after(None)
    got, st = table_after(torch.cuda.Stream())
    assert len(want) > 1000 and np.array_equal(got, want)
    assert (st["inserted"], st["distinct"]) == (want_st["inserted"], want_st["distinct"])


@pytest.mark.parametrize("merge", ["runs", "general", "shuffled", "runs_gaps"])
@pytest.mark.parametrize("path", ["direct", "partitioned"])
@pytest.mark.parametrize("k,mode,G", [(31, 2, 2), (31, 0, 3), (51, 2, 4), (63, 1, 2), (127, 0, 2)])
def test_preaggregated_merge_union(tmp_path, monkeypatch, k, mode, G, path, merge):
    """Pre-aggregated sharding (ShardedCounter's path): each emulated rank counts its own
    reads locally, routes its table as {key, count} records by owner, and every owner adds
    the records it receives; the owners' outputs are disjoint and their union is the
    oracle's count of the whole input (transforms applied to the merged counts).
    merge: runs = the region-sorted groups in one level-3 pass (kc_insert_counts_runs_device),
    general = the partitioned merge insert, shuffled = runs on unsorted groups (the device
    check sends them to the general insert)."""
    monkeypatch.setenv("KC_INSERT_PATH", path)  # local counting and the merge insert
    n_reads = 20000
    per = n_reads // G
    images = []
    for r in range(G):
        fa = tmp_path / f"r{r}.fasta"
        cnt = per if r < G - 1 else n_reads - per * (G - 1)
        # a small genome: every k-mer occurs on several ranks, so the merge adds counts
        subprocess.run([GEN, str(fa), str(n_reads), "150", "20000", "--first", str(r * per), "--count", str(cnt)],
                       check=True)
        images.append(_image(str(fa)))
    whole = tmp_path / "all.fasta"
    with open(whole, "wb") as f:
        for data, _ in images:
            f.write(data)
    engines = [DeviceEngine(ka.Config(k=k, mode=mode, table_slots=400000, min_abundance=1)) for _ in range(G)]
    W = engines[0].W
    stream = torch.cuda.current_stream().cuda_stream
    routed = []
    for r, (data, img) in enumerate(images):
        engines[r].reset()
        engines[r].count(img.data_ptr(), ka.plan_chunks(data, k, ka.FMT_FASTA, chunk_size=128 * 1024), ka.FMT_FASTA,
                         stream)
        recs, counts = engines[r].route_table(G, stream)
        torch.cuda.synchronize()
        assert sum(counts) == engines[r].kc.finish()["distinct"]
        routed.append((recs[: sum(counts) * (W + 1)].clone(), counts))
    for d in range(G):
        parts = []
        for recs, counts in routed:
            lo = sum(counts[:d]) * (W + 1)
            parts.append(recs[lo:lo + counts[d] * (W + 1)])
        if merge == "shuffled":
            parts = [p.view(-1, W + 1)[torch.randperm(p.numel() // (W + 1), device=p.device)].reshape(-1)
                     for p in parts]
        if merge == "runs_gaps":  # empty groups before, between and after the senders' groups
            empty = parts[0][:0]
            parts = [empty] + [x for p in parts for x in (p, empty)]
        recv = torch.cat(parts)
        gc = [p.numel() // (W + 1) for p in parts] if merge != "general" else None
        engines[d].insert_counts(recv, recv.numel() // (W + 1), stream, group_counts=gc)
        torch.cuda.synchronize()
        assert engines[d].owner_table().finish()["inserted"] == int(recv.view(-1, W + 1)[:, W].sum())
    shard_lines = [set(e.owner_table().lines()) for e in engines]
    kmers = [set(l.rsplit(" ", 1)[0] for l in s) for s in shard_lines]
    for a in range(G):
        for b in range(a + 1, G):
            assert not (kmers[a] & kmers[b]), "a k-mer has two owners"
    union = set().union(*shard_lines)
    out = tmp_path / "oracle.txt"
    oracle_count(str(whole), k, ["-m", str(mode), "-a", "1"], out)
    assert sorted_digest_lines(union) == sorted_digest_file(out)


@pytest.mark.parametrize("k,mode,G", [(31, 2, 2), (51, 0, 3)])
def test_two_merges_route_only_new_counts(tmp_path, k, mode, G):
    """A job that merges twice (count, merge, count more, merge): after routing, the local
    table is cleared (kc_clear_table) but keeps its window counters, so the second merge
    routes only what was counted after the first and the owners' union is still exact."""
    n_reads = 12000
    per = n_reads // G
    images = []
    for r in range(G):
        fa = tmp_path / f"r{r}.fasta"
        cnt = per if r < G - 1 else n_reads - per * (G - 1)
        subprocess.run([GEN, str(fa), str(n_reads), "150", "20000", "--first", str(r * per), "--count", str(cnt)],
                       check=True)
        images.append(_image(str(fa)))
    whole = tmp_path / "all.fasta"
    with open(whole, "wb") as f:
        for data, _ in images:
            f.write(data)
    engines = [DeviceEngine(ka.Config(k=k, mode=mode, table_slots=400000, min_abundance=1)) for _ in range(G)]
    W = engines[0].W
    stream = torch.cuda.current_stream().cuda_stream
    plans = [ka.plan_chunks(data, k, ka.FMT_FASTA, chunk_size=64 * 1024) for data, _ in images]
    per_windows = [len(data.split(b"\n")) // 2 * (150 - k + 1) for data, _ in images]
    for e in engines:
        e.reset()
    for phase in range(2):
        routed = []
        for r, (data, img) in enumerate(images):
            ch = plans[r]
            half = ch[: len(ch) // 2] if phase == 0 else ch[len(ch) // 2:]
            engines[r].count(img.data_ptr(), half, ka.FMT_FASTA, stream)
            recs, counts = engines[r].route_table(G, stream)
            engines[r].clear_local()
            torch.cuda.synchronize()
            routed.append((recs[: sum(counts) * (W + 1)].clone(), counts))
        for d in range(G):
            recv = torch.cat([recs[sum(c[:d]) * (W + 1):(sum(c[:d]) + c[d]) * (W + 1)] for recs, c in routed])
            engines[d].insert_counts(recv, recv.numel() // (W + 1), stream)
            torch.cuda.synchronize()
    for r in range(G):  # the cleared local tables kept their window counters
        assert engines[r].kc.finish()["windows"] == per_windows[r]
    union = set().union(*[set(e.owner_table().lines()) for e in engines])
    out = tmp_path / "oracle.txt"
    oracle_count(str(whole), k, ["-m", str(mode), "-a", "1"], out)
    assert sorted_digest_lines(union) == sorted_digest_file(out)


def merge_rule(parts, nparts, n, layout):
    """kc_bloom_merge_device's rule (checker restatement): filter 1 = OR, filter 2 = OR |
    filter-1 bits set in >= 2 copies; blocked = words 0-7 / 8-15 of 16-word blocks,
    reference = even / odd bits of every word."""
    import numpy as np

    p = parts[: nparts * n].reshape(nparts, n).astype(np.uint32)
    if layout == "blocked":
        p = p.reshape(nparts, n // 16, 2, 8)
        f1, f2 = p[:, :, 0], p[:, :, 1]
    else:
        f1, f2 = p & np.uint32(0x55555555), p & np.uint32(0xAAAAAAAA)
    once = np.zeros_like(f1[0])
    twice = np.zeros_like(f1[0])
    for i in range(nparts):
        twice |= once & f1[i]
        once |= f1[i]
    orf2 = np.bitwise_or.reduce(f2, axis=0)
    if layout == "blocked":
        return np.stack([once, orf2 | twice], axis=1).reshape(-1)
    return (once | orf2 | (twice << np.uint32(1))).reshape(-1)


@pytest.mark.parametrize("layout", ["blocked", "reference"])
def test_bloom_merge_kernel(monkeypatch, layout):
    """kc_bloom_merge_device against its restatement on random filter copies."""
    import numpy as np

    if layout == "reference":
        monkeypatch.setenv("KC_BLOOM_LAYOUT", "reference")
    kc = ka.KmerCounter(ka.Config(k=31, mode=2, bf_enable=True, est_unique=100000, fpr=0.01))
    rng = np.random.default_rng(5)
    for nparts in (1, 2, 3, 5):
        n = 16 * 37
        parts = rng.integers(0, 1 << 32, size=nparts * n, dtype=np.uint64).astype(np.uint32)
        parts &= rng.integers(0, 1 << 32, size=parts.size, dtype=np.uint64).astype(np.uint32)  # sparser
        dp = torch.from_numpy(parts.view(np.int32)).cuda()
        out = torch.empty(n, dtype=torch.int32, device="cuda")
        kc.bloom_merge_device(dp.data_ptr(), nparts, n, out.data_ptr(), 0)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        assert (got == merge_rule(parts, nparts, n, layout)).all()
    kc.close()


def _emulated_bloom_job(tmp_path, k, mode, G, n_reads, genome, est_unique):
    """G emulated ranks through ShardedCounter's owner-sharded Bloom flow: every
    rank counts its reads ungated, its local table's records go to their owners, and each
    owner runs the Bloom pass over the records it received (kc_bloom_records_device), sizes its
    table from its own new_in_second, and counts the same records behind its gate
    (kc_count_records_device).  Returns (engines, whole input, summed new_in_second)."""
    per = n_reads // G
    images = []
    for r in range(G):
        fa = tmp_path / f"r{r}.fasta"
        cnt = per if r < G - 1 else n_reads - per * (G - 1)
        subprocess.run([GEN, str(fa), str(n_reads), "150", str(genome), "--first", str(r * per), "--count", str(cnt)],
                       check=True)
        images.append(_image(str(fa)))
    whole = tmp_path / "all.fasta"
    with open(whole, "wb") as f:
        for data, _ in images:
            f.write(data)
    cfg = ka.Config(k=k, mode=mode, bf_enable=True, est_unique=est_unique, fpr=0.01, min_abundance=2)
    engines = [DeviceEngine(cfg, local_slots=4 * n_reads * 150, world=G) for _ in range(G)]
    W = engines[0].W
    stream = torch.cuda.current_stream().cuda_stream
    plans = [ka.plan_chunks(data, k, ka.FMT_FASTA, chunk_size=128 * 1024) for data, _ in images]
    routed = []
    for e, (data, img), ch in zip(engines, images, plans):
        e.reset()
        e.bloom(img.data_ptr(), ch, ka.FMT_FASTA, stream)  # the ungated local count
        recs, counts = e.route_table(G, stream)
        torch.cuda.synchronize()
        routed.append((recs[: sum(counts) * (W + 1)].clone(), counts))
    nis = 0
    for d in range(G):
        recv = torch.cat([recs[sum(c[:d]) * (W + 1):(sum(c[:d]) + c[d]) * (W + 1)] for recs, c in routed])
        n = recv.numel() // (W + 1)
        engines[d].bloom_records(recv, n, stream)
        nis += engines[d].owner_bloom_finalize()
        engines[d].count_records(recv, n, stream)
        torch.cuda.synchronize()
    return engines, whole, nis


@pytest.mark.parametrize("k,mode,G", [(31, 2, 2), (51, 0, 3), (95, 2, 4)])
def test_sharded_bloom_emulated_ranks(tmp_path, k, mode, G):
    """Owner-sharded Bloom filter: the owners' union of T(c) >= 2 lines equals the
    oracle's count of the whole input (the gate passes every k-mer seen twice, also when its
    two sightings are on two ranks), the owners are disjoint, and the owners' new_in_second
    sums to about the number of distinct k-mers seen twice.  (Blocked filter layout: the
    reference layout hashes the Rabin-Karp root, which the exchanged records do not carry.)"""
    engines, whole, nis = _emulated_bloom_job(tmp_path, k, mode, G, 12000, 20000, 400000)
    lines = [set(e.owner_table().lines()) for e in engines]
    for a in range(G):
        for b in range(a + 1, G):
            assert not ({l.rsplit(" ", 1)[0] for l in lines[a]} & {l.rsplit(" ", 1)[0] for l in lines[b]})
    out = tmp_path / "oracle.txt"
    oracle_count(str(whole), k, ["-m", str(mode), "-a", "2"], out)
    assert sorted_digest_lines(set().union(*lines)) == sorted_digest_file(out)
    n2 = sorted_digest_file(out)[1]
    assert 0.9 * n2 <= nis <= 1.5 * n2, (nis, n2)  # (+ singletons whose filter-1 bits were all set by others)
    for e in engines:
        e.close()


class _OneRank:
    """torch.distributed stand-in for a one-rank group (no collective is issued at world 1)."""

    @staticmethod
    def get_world_size(group=None):
        return 1

    @staticmethod
    def get_rank(group=None):
        return 0


@pytest.mark.parametrize("k,side", [(31, False), (63, False), (31, True)])
def test_sharded_counter_bloom_one_rank(tmp_path, k, side):
    """ShardedCounter's own Bloom path on the HIP engine (bloom_device -> bloom_finalize ->
    count_device -> merge) at one rank: the oracle's T(c) >= 2 lines.  side: the caller's
    stream is not torch's current stream (bloom_finalize and merge order their collectives
    and kc_* calls on it, sharded.py _on_stream)."""
    from kaarme_amd.sharded import ShardedCounter

    fa = tmp_path / "r.fasta"
    subprocess.run([GEN, str(fa), "8000", "150", "20000"], check=True)
    data, img = _image(str(fa))
    cfg = ka.Config(k=k, mode=2, bf_enable=True, est_unique=300000, fpr=0.01, min_abundance=2)
    sc = ShardedCounter(cfg, _OneRank())
    if side:
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        stream = s.cuda_stream
    else:
        stream = torch.cuda.current_stream().cuda_stream
    ch = ka.plan_chunks(data, k, ka.FMT_FASTA)
    sc.bloom_device(img.data_ptr(), ch, ka.FMT_FASTA, stream)
    nis = sc.bloom_finalize()
    sc.count_device(img.data_ptr(), ch, ka.FMT_FASTA, stream)
    st = sc.finish()
    assert st["new_in_second"] == nis > 0 and st["bf_windows"] == st["windows"]
    out = tmp_path / "oracle.txt"
    oracle_count(str(fa), k, ["-m", "2", "-a", "2"], out)
    assert sorted_digest_lines(sc.lines()) == sorted_digest_file(out)


@pytest.mark.parametrize("G", [2, 4, 8])
def test_sharded_bloom_excess_at_design_load(tmp_path, G):
    """with the filter sharded by owner, a k-mer seen once meets one filter
    (its owner's, sized for the owner's 1/G share of -u) holding the insertions one GPU's filter
    would hold, so the singletons that pass the gate are as few as with one filter -- not the
    1.5 / 2.6 / 3.8 % of the former bit-level merge of G whole filters at G = 2 / 4 / 8.  At -u
    = the true distinct count (the filter's design load): counts >= 2 exact, the singleton pass
    rate of the G owners within noise of the single filter's, and each owner's filter 1/G of
    the single filter (next power of two).  Written to gpurun_out/bloom_excess_G<G>.json."""
    import json

    out = tmp_path / "oracle.txt"
    n_reads, genome = 16000, 40000
    fa = tmp_path / "whole.fasta"
    subprocess.run([GEN, str(fa), str(n_reads), "150", str(genome)], check=True)
    oracle_count(str(fa), 31, ["-m", "2", "-a", "1"], out)
    distinct = sorted_digest_file(out)[1]
    engines, whole, nis = _emulated_bloom_job(tmp_path, 31, 2, G, n_reads, genome, distinct)
    lines = set().union(*[set(e.owner_table().lines()) for e in engines])
    owner_distinct = sum(e.owner_table().finish()["distinct"] for e in engines)
    owner_bits = [e.owner_table().bloom_info()["bits"] for e in engines]
    oracle_count(str(whole), 31, ["-m", "2", "-a", "2"], out)
    solid = sorted_digest_file(out)
    assert sorted_digest_lines(lines) == solid
    singletons = distinct - solid[1]
    excess = (owner_distinct - solid[1]) / max(1, singletons)
    # the same job on one GPU, one filter of -u bits: its singleton pass rate
    data, img = _image(str(whole))
    cfg = ka.Config(k=31, mode=2, bf_enable=True, est_unique=distinct, fpr=0.01, min_abundance=2)
    with ka.KmerCounter(cfg) as kc:
        ch = ka.plan_chunks(data, 31, ka.FMT_FASTA)
        kc.bloom_device(img.data_ptr(), ch, ka.FMT_FASTA)
        kc.bloom_finalize()
        kc.count_device(img.data_ptr(), ch, ka.FMT_FASTA)
        st1 = kc.finish()
        single_bits = kc.bloom_info()["bits"]
    excess1 = (st1["distinct"] - solid[1]) / max(1, singletons)
    os.makedirs(os.path.join(REPO, "gpurun_out"), exist_ok=True)
    with open(os.path.join(REPO, "gpurun_out", f"bloom_excess_G{G}.json"), "w") as f:
        json.dump({"G": G, "distinct": distinct, "solid": solid[1], "owner_distinct": owner_distinct,
                   "singletons_passed_frac": excess, "single_filter_singletons_passed_frac": excess1,
                   "nis": nis, "owner_filter_bits": owner_bits, "single_filter_bits": single_bits}, f)
    assert all(b * G <= 2 * single_bits for b in owner_bits), (owner_bits, single_bits)
    assert excess <= 1.5 * excess1 + 0.005, (excess, excess1)
    for e in engines:
        e.close()


def _routed_groups(kc, G):
    """kc_route_table_device's records, each owner's group as a sorted array."""
    import numpy as np

    counts = kc.route_table_device(G, 0, 0)
    n = sum(counts)
    W = ka.words_for_k(kc.cfg.k)
    out = torch.empty(max(1, n) * (W + 1), dtype=torch.int64, device="cuda")
    counts2 = kc.route_table_device(G, out.data_ptr(), max(1, n))
    assert counts2 == counts
    st = kc.finish()
    recs = out[: n * (W + 1)].view(-1, W + 1).cpu().numpy()
    groups, lo = [], 0
    for c in counts:
        g = recs[lo:lo + c]
        groups.append(g[np.lexsort(g.T[::-1])])
        lo += c
    return counts, groups, st


@pytest.mark.parametrize("k,path,batch_mib", [(31, "partitioned", 0), (31, "partitioned", 8), (51, "partitioned", 0),
                                               (127, "partitioned", 0), (31, "direct", 0)])
def test_route_hint_keeps_owner_counts(monkeypatch, k, path, batch_mib):
    """kc_route_hint: the level-3 passes keep the per-block owner counts, so
    kc_route_table_device runs no count pass -- and routes the same records as without the hint:
    one batch (fresh level 3), several batches (level 3 over a written table), after
    kc_clear_table, a route to another number of owners; the direct path keeps none."""
    import numpy as np

    monkeypatch.setenv("KC_INSERT_PATH", path)
    G = 4
    lib = ka.load_library()
    N, L = 200_000, 150
    nbytes = lib.kc_synth_bytes(0, N, L, 0)
    img = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert lib.kc_synth_device(img.data_ptr(), 0, N, 5, 2_000_000, L, 0, 0.002, 0.0, 0) == 0
    torch.cuda.synchronize()
    chunks = ka.plan_chunks_device(img.data_ptr(), nbytes, k, ka.FMT_FASTA, chunk_size=1 << 20)
    cfg = ka.Config(k=k, mode=2, table_slots=6_000_000, min_abundance=1, batch_bytes=batch_mib << 20)
    with ka.KmerCounter(cfg) as want_kc, ka.KmerCounter(cfg) as kc:
        kc.route_hint(G)
        for job in range(2):
            for c in (want_kc, kc):
                if job:
                    c.clear_table()
                c.count_device(img.data_ptr(), chunks if not job else chunks[: len(chunks) // 2], ka.FMT_FASTA)
            wc, wg, _ = _routed_groups(want_kc, G)
            gc, gg, st = _routed_groups(kc, G)
            assert gc == wc and sum(gc) > 0
            assert all(np.array_equal(a, b) for a, b in zip(gg, wg))
            # two routes per job (the count-only call and the scatter): after level 3 both take the
            # kept counts; after the direct path the first runs the count pass, which the second reuses
            assert st["route_counts_kept"] == (2 if path == "partitioned" else 1) * (job + 1), st
        # another owner count: the count pass runs, the records are the same
        wc3, wg3, _ = _routed_groups(want_kc, 3)
        gc3, gg3, st3 = _routed_groups(kc, 3)
        assert gc3 == wc3 and all(np.array_equal(a, b) for a, b in zip(gg3, wg3))
        assert st3["route_counts_kept"] == st["route_counts_kept"]


def test_route_hint_bloom_job_from_kept_partitions(monkeypatch):
    """A Bloom job whose counting pass runs from the Bloom pass's kept partitions (its fresh gated
    level 3) keeps the owner counts too; the same records as without the hint."""
    import numpy as np

    monkeypatch.setenv("KC_INSERT_PATH", "partitioned")
    G, k = 2, 51
    lib = ka.load_library()
    N, L = 200_000, 150
    nbytes = lib.kc_synth_bytes(0, N, L, 0)
    img = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert lib.kc_synth_device(img.data_ptr(), 0, N, 6, 2_000_000, L, 0, 0.002, 0.0, 0) == 0
    torch.cuda.synchronize()
    chunks = ka.plan_chunks_device(img.data_ptr(), nbytes, k, ka.FMT_FASTA)
    cfg = ka.Config(k=k, mode=2, min_abundance=2, bf_enable=True, est_unique=6_000_000, fpr=0.01)
    res = []
    for hint in (False, True):
        with ka.KmerCounter(cfg) as kc:
            if hint:
                kc.route_hint(G)
            kc.bloom_device(img.data_ptr(), chunks, ka.FMT_FASTA)
            kc.bloom_finalize()
            kc.count_device(img.data_ptr(), chunks, ka.FMT_FASTA)
            res.append(_routed_groups(kc, G))
    (wc, wg, _), (gc, gg, st) = res
    assert st["reused_passes"] == 1 and st["route_counts_kept"] == 2, st
    # the gate lets a run-dependent few singletons through (concurrent insertions):
    # the records of k-mers counted at least twice are the same
    solid = lambda g: g[g[:, -1] >= 2]
    assert all(np.array_equal(solid(a), solid(b)) for a, b in zip(gg, wg))
    # (the singletons through the gate -- filter-2 false positives, ~1 % of the error k-mers -- differ
    # by run: the records per owner agree to 1 %; 0.1 % failed one whole-suite run in four)
    assert all(abs(a - b) < 0.01 * b for a, b in zip(gc, wc))
