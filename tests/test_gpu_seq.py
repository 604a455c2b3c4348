"""GPU: sequence queries of the counted table -- kc_text_counts* (T(c) of the k-mer at every position
of a text) and kc_seq_stats* (per-sequence statistics of those counts).

Expected values never come from the code under test: the C oracle's ``-a 1`` output becomes a
{canonical k-mer: count} dictionary and the pure-Python model of seq_model.py applies it.  All
comparisons are exact.  The tables are counted from kc_gen reads as in test_gpu_query.py (3000 x
max(150, k + 100) bp over a 40 kbp genome, 0.2 % errors) or from golden inputs.
"""
import ctypes
import subprocess

import numpy as np
import pytest

from conftest import GEN, load_cases, oracle_count
import kaarme_amd as ka
import seq_model
from seq_model import NO_KMER

pytestmark = pytest.mark.gpu

# W = 1, 1, 2, 2, 2, 3, 4, 5, 7, 8, 15 (windows per thread 16, 8, 8, 4: run_width of kc_internal.h)
KS = [5, 31, 32, 33, 63, 64, 127, 128, 200, 255, 479]
RUNW = {31: 16, 33: 8}
KC_ERR_ARG, KC_ERR_STATE = -1, -4
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
SENT = 0x5EA7BEEF


def _seqs_of(path):
    with open(path, "rb") as f:
        return [ln.rstrip(b"\n") for ln in f if not ln.startswith(b">")]


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """k -> (path of the generated reads, their sequences), made once per read length."""
    work = tmp_path_factory.mktemp("seq_reads")
    cache = {}

    def get(k):
        L = max(150, k + 100)
        if L not in cache:
            fa = work / f"r{L}.fasta"
            subprocess.run([GEN, str(fa), "3000", str(L), "40000", "-e", "0.002"], check=True)
            cache[L] = (str(fa), _seqs_of(fa))
        return cache[L]

    return get


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    """The 40 kbp genome the reads come from: one error-free read of the genome's length."""
    fa = tmp_path_factory.mktemp("seq_genome") / "g.fasta"
    subprocess.run([GEN, str(fa), "1", "40000", "40000", "-e", "0"], check=True)
    (g,) = _seqs_of(fa)
    assert len(g) == 40000
    return g


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    """(path, k, oracle args) -> {canonical k-mer: count} of the oracle's output (run once each)."""
    work = tmp_path_factory.mktemp("seq_oracle")
    cache = {}

    def get(path, k, args=("-m", "2", "-a", "1")):
        key = (path, k, tuple(args))
        if key not in cache:
            out = work / f"o{len(cache)}.txt"
            oracle_count(path, k, list(args), out)
            cache[key] = seq_model.oracle_dict(out)
        return cache[key]

    return get


@pytest.fixture(scope="module")
def counted(reads, oracle):
    """k -> (counter over the reads of k, the oracle's dictionary); shared by the tests that only read."""
    cache = {}

    def get(k):
        if k not in cache:
            kc, st = ka.count_file(reads(k)[0], k, mode=2, min_abundance=1, table_slots=1 << 20)
            d = oracle(reads(k)[0], k)
            assert st["distinct"] == len(d) > 0
            cache[k] = (kc, d)
        return cache[k]

    yield get
    for kc, _ in cache.values():
        kc.close()


def _random_seq(rng, n):
    return bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=n))


def _mixed_text(seqs, k, seed):
    """~200 counted reads and 50 random ones (mostly absent k-mers), '\\n' between them, with
    lower-case stretches and some N."""
    rng = np.random.default_rng(seed)
    L = len(seqs[0])
    parts = [seqs[i] for i in rng.choice(len(seqs), size=200, replace=False)] + [_random_seq(rng, L) for _ in range(50)]
    parts = [parts[i] for i in rng.permutation(len(parts))]
    text = bytearray(b"\n".join(parts) + b"\n")
    for _ in range(40):  # lower-case stretches
        a = int(rng.integers(0, len(text) - 60))
        text[a:a + 60] = bytes(text[a:a + 60]).lower()
    for p in rng.integers(0, len(text), size=60):  # single N, and a few runs of them
        text[int(p)] = ord("N")
    for p in rng.integers(0, len(text) - 10, size=5):
        text[int(p):int(p) + 10] = b"NNNNNnnnnn"
    return bytes(text)


def _want(text, k, d):
    return np.array(seq_model.text_counts(text, k, d), dtype=np.uint32)


def _stats_rows(stats):
    return [dict(zip(seq_model.FIELDS, (int(x) for x in row))) for row in stats.tolist()]


# ---- 1. every key width ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_text_counts_every_key_width(k, reads, counted):
    kc, d = counted(k)
    text = _mixed_text(reads(k)[1], k, k)
    want = _want(text, k, d)
    valid = want != NO_KMER
    assert valid.sum() > 1000 and (want[valid] > 0).sum() > 1000
    assert k < 16 or (want[valid] == 0).sum() > 1000  # (every 5-mer is in the table)
    got = kc.text_counts(text)
    assert got.dtype == np.uint32 and got.shape == (len(text),)
    assert ((got == NO_KMER) == ~valid).all()
    assert (got == want).all()
    # the other strand: the window at p is the window at n - p - k of the reverse complement
    back = kc.text_counts(text.translate(COMP)[::-1])
    assert (back[back != NO_KMER] == want[valid][::-1]).all()


# ---- 2. shapes where the kernels can go wrong ------------------------------------------------------
def _plain_text(seqs, n):
    """>= n bytes of counted reads joined with nothing between them: no break at all"""
    out, i = b"", 0
    while len(out) < n:
        out += seqs[i]
        i += 1
    return out


@pytest.mark.parametrize("k", [31, 33])
def test_text_counts_lengths(k, reads, counted):
    kc, d = counted(k)
    base = bytearray(_plain_text(reads(k)[1], 4200))
    base[40] = ord("n")
    base[2000:2003] = b"\n>x"
    base = bytes(base)
    r = 32 * RUNW[k]
    for n in sorted({0, 1, k - 1, k, k + 1, 31, 32, 33, 63, 64, 65, r - 1, r, r + 1, 4095, 4096, 4097}):
        text = base[:n]  # truncated on the host: the windows over the cut are gone
        got = kc.text_counts(text)
        assert got.shape == (n,), n
        assert (got == _want(text, k, d)).all(), n
        if n >= k:
            assert (got[n - k + 1:] == NO_KMER).all(), n


@pytest.mark.parametrize("k", [31, 33])
def test_text_counts_breaks_and_no_breaks(k, reads, counted):
    kc, d = counted(k)
    plain = _plain_text(reads(k)[1], 1500)
    want = _want(plain, k, d)
    assert (want[:len(plain) - k + 1] != NO_KMER).all()  # no break at all
    assert (kc.text_counts(plain) == want).all()
    for pos in (64, 95, 0, 31, 32, len(plain) - 1):  # first / last byte of a packed word, the ends
        t = bytearray(plain)
        t[pos] = ord("N")
        t = bytes(t)
        assert (kc.text_counts(t) == _want(t, k, d)).all(), pos
    for filler in (b"N", b"\n", b"x"):  # all breaks
        assert (kc.text_counts(filler * 700) == NO_KMER).all()


@pytest.mark.parametrize("k", [31, 33])
def test_text_counts_device_unaligned_pointer(k, reads, counted):
    import torch
    kc, d = counted(k)
    text = _mixed_text(reads(k)[1], k, 7)[:5000]
    buf = torch.frombuffer(bytearray(b"ACGT" * 8 + text + b"ACGT" * 8), dtype=torch.uint8).cuda()
    for shift, n in ((1, 3000), (3, 4097), (13, 1001), (16, 2048), (2, 33)):
        sub = buf[32 + shift:32 + shift + n]  # (the text starts at byte 32 of a 256-byte-aligned buffer)
        want = _want(text[shift:shift + n], k, d)
        out = torch.full((n + 32,), SENT, dtype=torch.int32, device="cuda")
        kc.text_counts_device(sub.data_ptr(), n, out.data_ptr() + 16 * 4)
        torch.cuda.synchronize()
        res = out.cpu().numpy().view(np.uint32)
        assert (res[:16] == SENT).all() and (res[16 + n:] == SENT).all(), (shift, n)
        assert (res[16:16 + n] == want).all(), (shift, n)
        # an output array at a 4-byte, not 16-byte, boundary
        kc.text_counts_device(sub.data_ptr(), n, out.data_ptr() + 13 * 4)
        torch.cuda.synchronize()
        res = out.cpu().numpy().view(np.uint32)
        assert (res[13:13 + n] == want).all() and (res[:13] == SENT).all(), (shift, n)


@pytest.mark.parametrize("k", [31, 33])
def test_text_counts_on_a_side_stream_then_more_counting(k, reads, oracle):
    """The query runs on the caller's stream; counting the same reads again on the context follows it:
    the first answer holds the counts, the second twice the counts."""
    import torch
    path, seqs = reads(k)
    d = oracle(path, k)
    kc, _ = ka.count_file(path, k, mode=2, min_abundance=1, table_slots=1 << 20)
    with kc:
        text = _mixed_text(seqs, k, 11)
        want = _want(text, k, d)
        src = torch.frombuffer(bytearray(text), dtype=torch.uint8).pin_memory()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dt = torch.empty(len(text), dtype=torch.uint8, device="cuda")
            dt.copy_(src, non_blocking=True)
            out = torch.full((len(text),), -2, dtype=torch.int32, device="cuda")
            kc.text_counts_device(dt.data_ptr(), len(text), out.data_ptr(), stream=s.cuda_stream)
        with open(path, "rb") as f:
            image = f.read()
        for off, ln, bh in ka.plan_chunks(image, k, ka.FMT_FASTA):
            kc.count_chunk(image[off:off + ln], ka.FMT_FASTA, bool(bh))
        again = kc.text_counts(text)
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == want).all()
        valid = want != NO_KMER
        assert (again[valid] == np.minimum(2 * want[valid].astype(np.int64), 16383)).all()
        assert (again[~valid] == NO_KMER).all()


# ---- 3. per-sequence statistics --------------------------------------------------------------------
def _stat_seqs(seqs, genome, k, rng):
    r = seqs[0]
    out = [b"", r[:k - 1], r[:k], r[:k + 1], r[:k + 2]]         # 0, 0, 1, 2, 3 windows
    out += seqs[10:310]                                         # the wave form
    out += [genome, genome.translate(COMP)[::-1][:20011]]       # the workgroup form (even / odd windows)
    out += [_random_seq(rng, 300), b"N" * 200, b"n" * (k + 5), r[:60] + b"N" + r[61:]]
    out += [genome[100:2148], genome[100:2149]]                 # 2048 and 2049 bytes: the two sides of the threshold
    return out


@pytest.mark.parametrize("k", [31, 33])
def test_seq_stats(k, reads, genome, counted):
    kc, d = counted(k)
    seqs = _stat_seqs(reads(k)[1], genome, k, np.random.default_rng(k))
    text, off = ka.pack_sequences(seqs)
    counts = {}
    for solid_min in (0, 1, 2, 16383):
        got = kc.seq_stats(seqs, solid_min=solid_min)
        assert got.dtype == ka.SEQ_STAT_DTYPE and len(got) == len(seqs)
        want = seq_model.seq_stats(text, off, k, d, solid_min)
        assert _stats_rows(got) == want, solid_min
        counts[solid_min] = got
    w = counts[1]
    assert w["windows"][:5].tolist() == [0, 0, 1, 2, 3]
    assert w["windows"][305] == 40000 - k + 1 and w["present"][305] > 30000    # the genome
    assert (w["windows"][305] % 2, w["windows"][306] % 2) in ((0, 1), (1, 0))
    assert w["windows"][307] > 0 and w["present"][307] == 0 and w["max"][307] == 0    # all absent
    assert w["windows"][308] == 0 and w[308].tolist() == (0,) * 7                      # all N
    assert (counts[0]["solid"] == w["windows"]).all() and (w["solid"] == w["present"]).all()


@pytest.mark.parametrize("k", [31, 33])
def test_seq_stats_adjacent_sequences_share_no_window(k, reads, counted):
    import torch
    kc, d = counted(k)
    seqs = reads(k)[1]
    a, b, c = seqs[5], seqs[5][40:] + seqs[6][:40], seqs[7][:k]
    text = a + b + c + b"ACGTACGT"  # no separator bytes; the text runs on past the last offset
    off = np.array([0, len(a), len(a) + len(b), len(a) + len(b), len(a) + len(b) + len(c)], dtype=np.uint64)
    want = seq_model.seq_stats(text, off, k, d, 1)
    assert [w["windows"] for w in want] == [len(a) - k + 1, len(b) - k + 1, 0, 1]
    dt = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    out = torch.zeros(4 * 32, dtype=torch.uint8, device="cuda")
    kc.seq_stats_device(dt.data_ptr(), len(text), off, out.data_ptr(), solid_min=1)
    torch.cuda.synchronize()
    assert _stats_rows(out.cpu().numpy().view(ka.SEQ_STAT_DTYPE)) == want
    # the joints do hold k-mers: the text as one stream has a window at every position
    assert (kc.text_counts(text)[:len(text) - k + 1] != NO_KMER).all()
    # offsets that start past the beginning
    kc.seq_stats_device(dt.data_ptr(), len(text), off[1:], out.data_ptr(), solid_min=1)
    torch.cuda.synchronize()
    assert _stats_rows(out.cpu().numpy().view(ka.SEQ_STAT_DTYPE)[:3]) == want[1:]


@pytest.mark.parametrize("k", [31, 33])
def test_seq_stats_in_several_passes(k, reads, genome, counted, oracle):
    """A context with a 32 KiB staging batch runs the text in passes of at most 32 KiB cut at sequence
    boundaries -- the 40 kbp genome is a pass of its own length -- and text_counts in pieces of 32 KiB:
    the same answers as the single pass of the big-batch context, and as the model."""
    import torch
    path, seqs = reads(k)
    d = oracle(path, k)
    big, _ = counted(k)
    some = seqs[100:500] + [genome] + seqs[500:900] + [b"", b"N" * 50] + seqs[900:1000]
    text, off = ka.pack_sequences(some)
    kc, st = ka.count_file(path, k, mode=2, min_abundance=1, table_slots=1 << 20, chunk_size=16384,
                           batch_bytes=32768)
    with kc:
        assert st["distinct"] == len(d) and len(text) > 5 * 32768
        dt = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
        out = torch.zeros(len(some) * 32, dtype=torch.uint8, device="cuda")
        kc.seq_stats_device(dt.data_ptr(), len(text), off, out.data_ptr(), solid_min=2)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(ka.SEQ_STAT_DTYPE)
        assert (got == big.seq_stats(some, solid_min=2)).all()
        assert _stats_rows(got) == seq_model.seq_stats(text, off, k, d, 2)
        assert (kc.text_counts(text) == _want(text, k, d)).all()


# ---- 4. other tables ------------------------------------------------------------------------------
def test_wrapped_counts_of_mode_0(golden_input, oracle):
    """-m 0 on the golden poly-A input: its counts wrap mod 65536 (T(c) = c mod 65536)."""
    k = 25
    path = golden_input("edge.fasta")
    d = oracle(path, k, ("-m", "0", "-a", "1"))
    kc, st = ka.count_file(path, k, mode=0, min_abundance=1, table_slots=1 << 20)
    with kc:
        seqs = [s for s in _seqs_of(path) if s][:150]
        head = b"\n".join(seqs) + b"\n"
        text = head + b"A" * (k + 10) + b"\n" + b"t" * k
        want = _want(text, k, d)
        got = kc.text_counts(text)
        assert (got == want).all()
        polya = d[b"A" * k]
        assert got[len(text) - k] == polya and (got[len(head):len(head) + 11] == polya).all()
        assert max(len(s) for s in _seqs_of(path)) - k + 1 > 65536  # one poly-A line alone wraps the count
        stats = kc.seq_stats([b"A" * (k + 10), seqs[0]], solid_min=3)
        assert _stats_rows(stats) == seq_model.seq_stats(*ka.pack_sequences([b"A" * (k + 10), seqs[0]]), k, d, 3)
        assert stats["sum"][0] == 11 * polya


BLOOM_CASE = [c for c in load_cases()["cases"]
              if c["input"] == "reads_w60.fasta" and "-b" in c["args"] and c["args"][-2:] == ["-a", "1"]][0]


def test_text_counts_after_a_bloom_job(golden_input, oracle):
    """Behind the Bloom gate (-b -a 1) counts >= 2 are exact; a true singleton is absent or, where
    the filter let it pass, 1 (as test_gpu_parity.py's bf_singleton_check)."""
    a, k = BLOOM_CASE["args"], BLOOM_CASE["k"]
    mode = int(a[a.index("-m") + 1]) if "-m" in a else 2
    path = golden_input(BLOOM_CASE["input"])
    d = oracle(path, k, ("-m", str(mode), "-a", "1"))  # the exact counts
    kc, st = ka.count_file(path, k, mode=mode, min_abundance=1, bf_enable=True, est_unique=int(a[a.index("-u") + 1]))
    with kc:
        seqs = [s for s in _seqs_of(path) if s]
        text = b"\n".join(seqs)[:30000] + b"\n" + _random_seq(np.random.default_rng(1), 500)
        want = _want(text, k, d)
        got = kc.text_counts(text)
        exact = want != 1
        assert (want >= 2).sum() > 1000 and (want == 1).any() and (want == 0).any()
        assert (got[exact] == want[exact]).all()
        assert (got[~exact] <= 1).all()
        some = [text[i:i + 200] for i in range(0, 6000, 200)]
        stats = kc.seq_stats(some, solid_min=2)
        model = seq_model.seq_stats(*ka.pack_sequences(some), k, d, 2)
        assert stats["windows"].tolist() == [m["windows"] for m in model]
        assert stats["solid"].tolist() == [m["solid"] for m in model]


def test_seq_queries_after_clear_and_reset(reads, oracle):
    k = 31
    path, seqs = reads(k)
    d = oracle(path, k)
    kc, st = ka.count_file(path, k, mode=2, min_abundance=1, table_slots=1 << 20)
    with kc:
        text = _mixed_text(seqs, k, 3)[:20000]
        want = _want(text, k, d)
        before = kc.finish()
        assert (kc.text_counts(text) == want).all()
        assert _stats_rows(kc.seq_stats(seqs[:50])) == seq_model.seq_stats(*ka.pack_sequences(seqs[:50]), k, d, 1)
        assert kc.finish() == before == st  # the queries change no counter
        empty = np.where(want == NO_KMER, NO_KMER, 0).astype(np.uint32)
        for wipe in (kc.clear_table, kc.reset):
            wipe()
            assert (kc.text_counts(text) == empty).all()
            stats = kc.seq_stats(seqs[:50])
            assert not stats["present"].any() and not stats["sum"].any() and not stats["max"].any()
            assert (stats["windows"] == len(seqs[0]) - k + 1).all()


def test_seq_queries_need_a_table_and_good_arguments(counted):
    with ka.KmerCounter(ka.Config(k=31, bf_enable=True, est_unique=100000, min_abundance=1)) as kc:
        with pytest.raises(ka.KcError) as e:
            kc.text_counts(b"ACGT" * 20)
        assert e.value.code == KC_ERR_STATE
        with pytest.raises(ka.KcError) as e:
            kc.seq_stats([b"ACGT" * 20])
        assert e.value.code == KC_ERR_STATE
    kc, _ = counted(31)
    text = b"ACGT" * 25
    out = np.zeros(4, dtype=ka.SEQ_STAT_DTYPE)

    def call(offsets, n_bytes=len(text)):
        off = np.array(offsets, dtype=np.uint64)
        return kc.lib.kc_seq_stats(kc._ctx, text, n_bytes, off.ctypes.data, len(off) - 1, 1, out.ctypes.data)

    assert call([0, 50, 40, 100]) == KC_ERR_ARG          # decreasing
    assert call([0, 50, 101]) == KC_ERR_ARG              # past n_bytes
    assert call([0, 50, 100], n_bytes=99) == KC_ERR_ARG
    assert call([0, 50, 50, 100]) == 0 and out["windows"].tolist() == [20, 0, 20, 0]
    assert call([7]) == 0                                # n_seqs = 0
    assert kc.lib.kc_seq_stats(kc._ctx, text, len(text), None, 2, 1, out.ctypes.data) == KC_ERR_ARG
    assert kc.lib.kc_text_counts(kc._ctx, None, 0, None) == 0
    assert kc.lib.kc_text_counts(kc._ctx, None, 5, None) == KC_ERR_ARG
    assert kc.lib.kc_text_counts_device(kc._ctx, None, 0, None, None) == 0
    assert len(kc.text_counts(b"")) == 0 and len(kc.seq_stats([])) == 0
    assert ctypes.sizeof(ctypes.c_uint32) * 8 == ka.SEQ_STAT_DTYPE.itemsize
