"""GPU: read correction from the counted table -- kc_correct* (isolated base errors of a text fixed in
one device pass).

Expected values never come from the code under test: the C oracle's ``-a 1`` output becomes a
{canonical k-mer: count} dictionary and the pure-Python model of correct_model.py applies the rule
of include/kc_api.h to it.  All comparisons are exact.  The tables are counted from kc_gen reads as
in test_gpu_seq.py (3000 x max(150, k + 100) bp over a 40 kbp genome, 0.2 % errors), from golden
inputs or from small FASTA files written here.
"""
import ctypes
import subprocess

import numpy as np
import pytest

from conftest import GEN, load_cases, oracle_count
import kaarme_amd as ka
import correct_model
import seq_model
from seq_model import NO_KMER

pytestmark = pytest.mark.gpu

# W = 1, 1, 2, 2, 2, 3, 4, 5, 7, 8, 15 (the key widths of test_gpu_seq.py; every 5-mer is solid, so 15)
KS = [15, 31, 32, 33, 63, 64, 127, 128, 200, 255, 479]
KC_ERR_ARG, KC_ERR_STATE = -1, -4
COMP = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")
MARK_TILE = 1024  # positions per workgroup of k_correct_mark (kc_internal.h CORRECT_TILE)


def _seqs_of(path):
    with open(path, "rb") as f:
        return [ln.rstrip(b"\n") for ln in f if not ln.startswith(b">")]


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """k -> (path of the generated reads, their sequences), made once per read length."""
    work = tmp_path_factory.mktemp("cor_reads")
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
    fa = tmp_path_factory.mktemp("cor_genome") / "g.fasta"
    subprocess.run([GEN, str(fa), "1", "40000", "40000", "-e", "0"], check=True)
    (g,) = _seqs_of(fa)
    assert len(g) == 40000
    return g


@pytest.fixture(scope="module")
def oracle(tmp_path_factory):
    """(path, k, oracle args) -> {canonical k-mer: count} of the oracle's output (run once each)."""
    work = tmp_path_factory.mktemp("cor_oracle")
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


def _mixed_text(seqs, seed, n_counted=400):
    """(text, offsets): counted reads and 50 random ones, one per sequence with its newline, with
    lower-case stretches and scattered N."""
    rng = np.random.default_rng(seed)
    L = len(seqs[0])
    parts = [seqs[i] for i in rng.choice(len(seqs), size=n_counted, replace=False)] + \
            [_random_seq(rng, L) for _ in range(50)]
    parts = [parts[i] for i in rng.permutation(len(parts))]
    text, off = ka.pack_sequences(parts)
    text = bytearray(text)
    for _ in range(40):  # lower-case stretches
        a = int(rng.integers(0, len(text) - 60))
        text[a:a + 60] = bytes(text[a:a + 60]).lower()
    for p in rng.integers(0, len(text), size=60):  # single N, and a few runs of them
        text[int(p)] = ord("N")
    for p in rng.integers(0, len(text) - 10, size=5):
        text[int(p):int(p) + 10] = b"NNNNNnnnnn"
    return bytes(text), off


def _rows(stats):
    return [dict(zip(correct_model.FIELDS, (int(x) for x in row))) for row in stats.tolist()]


def _host(kc, text, off, solid_min=1, want_stats=True):
    """kc_correct on host arrays -> (output bytes, stats rows or None)"""
    off = np.ascontiguousarray(off, dtype=np.uint64)
    out = ctypes.create_string_buffer(max(len(text), 1))
    stats = np.full(len(off) - 1, 0xEE, dtype=np.uint8).repeat(16).view(ka.CORRECT_STAT_DTYPE)
    rc = kc.lib.kc_correct(kc._ctx, text, len(text), off.ctypes.data, len(off) - 1, solid_min, out,
                           stats.ctypes.data if want_stats else None)
    assert rc == 0, rc
    return out.raw[:len(text)], (_rows(stats) if want_stats else None)


def _device(kc, text, off, solid_min=1, shift=0, in_place=False, want_stats=True, stream=0):
    """kc_correct_device with the text (and the output) `shift` bytes into 256-byte-aligned buffers"""
    import torch
    off = np.ascontiguousarray(off, dtype=np.uint64)
    n = len(text)
    dt = torch.frombuffer(bytearray(b"#" * shift + text + b"#" * 16), dtype=torch.uint8).cuda()
    do = dt if in_place else torch.full((n + shift + 16,), ord("#"), dtype=torch.uint8, device="cuda")
    ds = torch.full((max(len(off) - 1, 1) * 16,), 0xEE, dtype=torch.uint8, device="cuda")
    kc.correct_device(dt.data_ptr() + shift, n, off, do.data_ptr() + shift, solid_min,
                      ds.data_ptr() if want_stats else 0, stream)
    torch.cuda.synchronize()
    res = do.cpu().numpy().tobytes()
    assert res[:shift] == b"#" * shift and res[shift + n:] == b"#" * 16  # nothing written around the output
    stats = ds.cpu().numpy().view(ka.CORRECT_STAT_DTYPE)[:len(off) - 1]
    return res[shift:shift + n], (_rows(stats) if want_stats else None)


def _plant(seq, positions):
    """seq with the base at each position replaced by the next one of ACGT"""
    s = bytearray(seq)
    for p in positions:
        s[p] = b"CGTA"[b"ACGT".index(s[p])]
    return bytes(s)


def _weak_sums(g, k, d, s):
    cnt = seq_model.text_counts(g, k, d)
    weak = np.array([c == NO_KMER or c < s for c in cnt[:len(g) - k + 1]])
    return np.concatenate([[0], np.cumsum(weak)])


def _solid_spots(g, k, d, s, need, gap):
    """`need` positions of g, at least `gap` apart, every window over which is solid in d"""
    csum = _weak_sums(g, k, d, s)
    out, p = [], k
    while p < len(g) - 2 * k and len(out) < need:
        if csum[p + 1] - csum[p - k + 1] == 0:  # the window starts p - k + 1 .. p
            out.append(p)
            p += gap
        else:
            p += 1
    assert len(out) == need
    return out


def _solid_stretch(g, k, d, s, length, lo=0):
    """a: every window of g[a : a + length] is solid in d"""
    csum = _weak_sums(g, k, d, s)
    for a in range(lo, len(g) - length):
        if csum[a + length - k + 1] == csum[a]:
            return a
    raise AssertionError("no solid stretch")


# ---- 1. every key width ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_correct_every_key_width(k, reads, counted):
    kc, d = counted(k)
    text, off = _mixed_text(reads(k)[1], k)
    want, wstats = correct_model.correct(text, off, k, d, 3)
    fixed = sum(s["corrected"] for s in wstats)
    assert fixed >= 10 and sum(s["candidates"] for s in wstats) - fixed >= 1000  # not vacuous
    assert fixed == sum(a != b for a, b in zip(want, text))
    got, gstats = _host(kc, text, off, 3)
    assert got == want
    assert gstats == wstats
    # the other strand: the reverse complement corrects to the reverse complement of the output
    n = len(text)
    back, bstats = _host(kc, text.translate(COMP)[::-1], (n - off.astype(np.int64))[::-1], 3)
    assert back == want.translate(COMP)[::-1]
    assert bstats == wstats[::-1]


# ---- 2. the hand cases ----------------------------------------------------------------------------
def _count_fasta(tmp_path, name, kmers, k, copies):
    fa = tmp_path / name
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, s) for i, s in enumerate(kmers * copies)))
    kc, st = ka.count_file(str(fa), k, mode=2, min_abundance=1, table_slots=1 << 16)
    return kc


@pytest.mark.parametrize("kmers,out,row", [
    ([b"TCGGTCA"], b"TCGGTCA", (7, 1, 0, 0)),
    ([b"TCGGTCA", b"CCGGTCA"], b"ACGGTCA", (7, 0, 1, 0)),
    ([b"TCGGTCA", b"ACGGTCT"], b"ACGGTCA", (7, 0, 0, 2)),
], ids=["one-works", "two-work", "two-accepted-closer-than-k"])
def test_hand_cases_k7(kmers, out, row, tmp_path):
    with _count_fasta(tmp_path, "t.fasta", kmers, 7, 5) as kc:
        want = dict(zip(correct_model.FIELDS, row))
        assert _device(kc, b"ACGGTCA", [0, 7], 2) == (out, [want])
        assert _host(kc, b"ACGGTCA", [0, 7], 2) == (out, [want])
        fixed, stats = kc.correct([b"ACGGTCA"], solid_min=2)
        assert fixed == [out] and _rows(stats) == [want]


def test_hand_case_lower_case_and_n(tmp_path):
    clean = b"ACGTTGCAAGGCTTAACCGGATATCGCGTAGCTAGGATCCTTGAC"
    bad = bytearray(clean)
    bad[20], bad[30] = ord("g"), ord("N")  # clean: A at 20
    want = bytearray(bad)
    want[20] = ord("a")
    with _count_fasta(tmp_path, "c.fasta", [clean], 7, 3) as kc:
        row = dict(zip(correct_model.FIELDS, (1, 1, 0, 0)))
        assert _device(kc, bytes(bad), [0, 45], 2) == (bytes(want), [row])
        assert _device(kc, bytes(bad), [0, 45], 3) == (bytes(want), [row])
        # from 4 on only AGGATCC / GGATCCT (one canonical k-mer, counted 6 times) is solid: of the 44 base
        # positions the 8 under the windows 33 and 34 are no candidates, and nothing can be corrected
        none = _device(kc, bytes(bad), [0, 45], 4)
        assert none == (bytes(bad), [dict(zip(correct_model.FIELDS, (36, 0, 0, 0)))])


# ---- 3. shapes where the kernels can go wrong ------------------------------------------------------
def _check(kc, text, off, k, d, s, min_fixed=0, **kw):
    want = correct_model.correct(text, off, k, d, s)
    assert sum(x["corrected"] for x in want[1]) >= min_fixed
    assert _device(kc, text, off, s, **kw) == want
    return want


@pytest.mark.parametrize("k", [31, 33])
def test_short_sequences(k, genome, counted):
    """lengths around k and 2k with an error at the first, the last and the middle base"""
    kc, d = counted(k)
    g0 = _solid_stretch(genome, k, d, 1, 2 * k, lo=500)
    seqs = []
    for L in (k - 1, k, k + 1, 2 * k - 2, 2 * k - 1, 2 * k):
        piece = genome[g0:g0 + L]
        seqs += [_plant(piece, [e]) for e in (0, L - 1, L // 2)] + [piece]
    text, off = ka.pack_sequences(seqs + [b"", b""])
    want = _check(kc, text, off, k, d, 1, min_fixed=15)
    assert [x["candidates"] for x in want[1][:4]] == [0, 0, 0, 0]  # k - 1 bases: no window
    assert [x["candidates"] for x in want[1][4:8]] == [k, k, k, 0]  # k bases: the one window covers them all
    assert _host(kc, text, off, 1) == want
    # the same sequences with no break byte between them
    joined = b"".join(seqs)
    joff = np.cumsum([0] + [len(s) for s in seqs])
    assert _check(kc, joined, joff, k, d, 1, min_fixed=15)[1] == want[1][:len(seqs)]


@pytest.mark.parametrize("k", [31, 33])
def test_mark_tile_edges(k, genome, counted):
    """sequences of T - 1, T and T + 1 bytes joined with no break byte, one error next to a tile edge
    so that the halo decides; the joints lie next to the edges too"""
    kc, d = counted(k)
    T = MARK_TILE
    g0 = _solid_stretch(genome, k, d, 1, 3 * T + 600, lo=2000)
    base = genome[g0:g0 + 3 * T + 600]
    lens = [T - 1, T, T + 1, 600 - 1]
    off = np.cumsum([0] + lens)
    fixed = 0
    for e in (T - 1, T, T + k - 2, 2 * T - (k - 1), 2 * T - 1, 2 * T, T - 2, T - k, 3 * T - 1, 3 * T + 1):
        want = _check(kc, _plant(base, [e]), off, k, d, 1)
        fixed += sum(x["corrected"] for x in want[1])
    assert fixed == 10
    # an error on either side of a joint: the two sequences share no window, both are corrected
    want = _check(kc, _plant(base, [T - 4, T + 1]), off, k, d, 1)
    assert [x["corrected"] for x in want[1]] == [1, 1, 0, 0]
    # as one sequence the two are closer than k: neither is corrected
    want = _check(kc, _plant(base, [T - 4, T + 1, 2 * T + 5]), [0, len(base)], k, d, 1)
    assert want[1][0]["corrected"] == 1
    # one sequence of 2049 bytes
    _check(kc, _plant(base[:2049], [5, 1024, 2040]), [0, 2049], k, d, 1, min_fixed=3)


@pytest.mark.parametrize("k", [31, 33])
def test_offsets_inside_the_text_and_empty_sequences(k, genome, counted):
    kc, d = counted(k)
    g0 = _solid_stretch(genome, k, d, 1, 700, lo=8000)
    base = genome[g0:g0 + 700]
    errs = [10, 150, 300, 450, 690]
    text = _plant(base, errs)
    off = [100, 100, 100, 400, 400, 600, 600]  # bytes before 100 and from 600 on belong to no sequence
    want = _check(kc, text, off, k, d, 1, min_fixed=3)
    assert want[0][:100] == text[:100] and want[0][600:] == text[600:]
    assert want[0][150] == base[150] and want[0][300] == base[300] and want[0][450] == base[450]
    assert [x["candidates"] for x in want[1]][0:2] == [0, 0]
    assert _host(kc, text, off, 1) == want
    # every sequence empty; offsets of one entry; no sequence at all
    assert _device(kc, text, [300, 300, 300], 2) == (text, [dict.fromkeys(correct_model.FIELDS, 0)] * 2)
    assert _device(kc, text, [7], 2)[0] == text
    assert _device(kc, text, [], 2)[0] == text


@pytest.mark.parametrize("k", [31, 33])
def test_odd_byte_addresses(k, reads, counted):
    kc, d = counted(k)
    text, off = _mixed_text(reads(k)[1], 7, n_counted=30)
    want = correct_model.correct(text, off, k, d, 2)
    assert sum(x["corrected"] for x in want[1]) >= 1
    for shift in (1, 3, 13):
        assert _device(kc, text, off, 2, shift=shift) == want
        assert _device(kc, text, off, 2, shift=shift, in_place=True) == want


@pytest.mark.parametrize("k", [31, 33])
def test_several_passes_and_a_sequence_longer_than_a_pass(k, reads, genome, counted, oracle):
    """A context with a 32 KiB staging batch runs the text in passes cut at sequence boundaries; the
    40 kbp genome with 20 planted substitutions at least k apart is a pass of its own, and all 20
    are corrected back."""
    path, seqs = reads(k)
    d = oracle(path, k)
    big, _ = counted(k)
    spots = _solid_spots(genome, k, d, 1, 20, 1500)
    bad = _plant(genome, spots)
    some = seqs[100:300] + [bad] + seqs[300:500] + [b"", b"N" * 50] + seqs[500:600]
    text, off = ka.pack_sequences(some)
    kc, st = ka.count_file(path, k, mode=2, min_abundance=1, table_slots=1 << 20, chunk_size=16384, batch_bytes=32768)
    with kc:
        assert st["distinct"] == len(d) and len(text) > 3 * 32768
        want = correct_model.correct(text, off, k, d, 1)
        a = int(off[200])
        assert want[0][a:a + 40000] == genome and want[1][200]["corrected"] == 20
        assert _device(kc, text, off, 1) == want
        assert _device(big, text, off, 1) == want  # one pass
        assert _host(kc, text, off, 1) == want


# ---- 4. in place ----------------------------------------------------------------------------------
def test_in_place_overlap_and_no_stats(reads, counted):
    import torch
    k = 31
    kc, d = counted(k)
    text, off = _mixed_text(reads(k)[1], 4, n_counted=100)
    want = correct_model.correct(text, off, k, d, 3)
    assert sum(x["corrected"] for x in want[1]) >= 2
    assert _device(kc, text, off, 3, in_place=True) == want
    assert _device(kc, text, off, 3, want_stats=False) == (want[0], None)
    assert _device(kc, text, off, 3, in_place=True, want_stats=False) == (want[0], None)
    assert _host(kc, text, off, 3, want_stats=False) == (want[0], None)
    # any other overlap is refused and writes nothing
    buf = torch.frombuffer(bytearray(text + b"#"), dtype=torch.uint8).cuda()
    offs = np.ascontiguousarray(off, dtype=np.uint64)
    for delta in (1, -1):
        src = buf.data_ptr() + (1 if delta < 0 else 0)
        rc = kc.lib.kc_correct_device(kc._ctx, src, len(text), offs.ctypes.data, len(offs) - 1, 3, src + delta, None, None)
        assert rc == KC_ERR_ARG
    torch.cuda.synchronize()
    assert buf.cpu().numpy().tobytes() == text + b"#"


# ---- 5. the guarantee -----------------------------------------------------------------------------
def test_guarantee_and_planted_truth(reads, genome, counted):
    """Every window of the GPU's output that holds a changed byte is solid by the model's counts, all
    other bytes are the input's; and against the genome no clean base of a counted read was changed
    (the simulation of the rule on this kind of data shows no miscorrection at k = 31; the bytes
    themselves are the model's in test_correct_every_key_width)."""
    k = 31
    kc, d = counted(k)
    seqs = reads(k)[1][:600]
    text, off = ka.pack_sequences(seqs)
    got, stats = _host(kc, text, off, 3)
    assert correct_model.guarantee_violations(text, got, off, k, d, 3) == []
    assert sum(x["corrected"] for x in stats) == sum(a != b for a, b in zip(got, text)) >= 50
    # where each read comes from: a 31-mer of it found in the genome, on either strand
    where = {genome[p:p + k]: p for p in range(len(genome) - k + 1)}
    L = len(seqs[0])
    located = changed = 0
    for i, r in enumerate(seqs):
        fixed = got[int(off[i]):int(off[i]) + L]
        for strand in (0, 1):
            rr, ff = (r, fixed) if not strand else (seq_model.revcomp(r), seq_model.revcomp(fixed))
            hit = [(where[rr[w:w + k]] - w) for w in range(0, L - k + 1, 17) if rr[w:w + k] in where]
            hit = [h for h in hit if 0 <= h <= len(genome) - L]
            if hit:
                truth = genome[hit[0]:hit[0] + L]
                located += 1
                for p in range(L):
                    if ff[p] != rr[p]:
                        changed += 1
                        assert rr[p] != truth[p] and ff[p] == truth[p], (i, p)  # an error, set to the truth
                break
    assert located >= 500 and changed >= 50


# ---- 6. modes and thresholds ----------------------------------------------------------------------
def test_mode_0_table(golden_input, oracle):
    k = 25
    path = golden_input("edge.fasta")
    d = oracle(path, k, ("-m", "0", "-a", "1"))
    kc, st = ka.count_file(path, k, mode=0, min_abundance=1, table_slots=1 << 20)
    with kc:
        seqs = [s for s in _seqs_of(path) if k <= len(s) <= 400][:60]
        seqs = [_plant(s, [len(s) // 2]) if i % 2 else s for i, s in enumerate(seqs)]
        seqs += [b"A" * 20 + b"C" + b"A" * 20]
        text, off = ka.pack_sequences(seqs)
        for s in (2, d[b"A" * k], d[b"A" * k] + 1):  # (the poly-A count has wrapped mod 65536)
            assert _host(kc, text, off, s) == correct_model.correct(text, off, k, d, s), s


def test_thresholds_of_a_saturated_table(golden_input, oracle):
    k = 25
    path = golden_input("edge.fasta")
    d = oracle(path, k, ("-m", "2", "-a", "1"))
    assert d[b"A" * k] == 16383
    kc, st = ka.count_file(path, k, mode=2, min_abundance=1, table_slots=1 << 20)
    with kc:
        read = b"A" * 20 + b"c" + b"A" * 20
        some = [s for s in _seqs_of(path) if k <= len(s) <= 400][:20]
        text, off = ka.pack_sequences([read] + some)
        assert _host(kc, text, off, 0) == _host(kc, text, off, 1) == correct_model.correct(text, off, k, d, 1)
        got = _host(kc, text, off, 16383)
        assert got == correct_model.correct(text, off, k, d, 16383)
        assert got[0][:41] == b"A" * 20 + b"a" + b"A" * 20 and got[1][0]["corrected"] == 1
        got = _host(kc, text, off, 16384)  # nothing is solid: candidates everywhere, nothing corrected
        assert got == correct_model.correct(text, off, k, d, 16384)
        assert got[0] == text and got[1][0] == dict(zip(correct_model.FIELDS, (41, 0, 0, 0)))


# ---- 7. states ------------------------------------------------------------------------------------
BLOOM_CASE = [c for c in load_cases()["cases"]
              if c["input"] == "reads_w60.fasta" and "-b" in c["args"] and c["args"][-2:] == ["-a", "1"]][0]


def _own_dict(kc):
    """the table's own content through kc_dump (not the code under test)"""
    return {seq_model.canonical(s.encode()): int(c) for s, c in (ln.split() for ln in kc.lines())}


def test_bloom_gated_table_and_table_op_result(golden_input):
    a, k = BLOOM_CASE["args"], BLOOM_CASE["k"]
    mode = int(a[a.index("-m") + 1]) if "-m" in a else 2
    path = golden_input(BLOOM_CASE["input"])
    with ka.KmerCounter(ka.Config(k=k, bf_enable=True, est_unique=100000, min_abundance=1)) as early:
        assert early.lib.kc_correct(early._ctx, b"ACGT" * 20, 80, (ctypes.c_uint64 * 2)(0, 80), 1, 1,
                                    ctypes.create_string_buffer(80), None) == KC_ERR_STATE
    kc, st = ka.count_file(path, k, mode=mode, min_abundance=1, bf_enable=True, est_unique=int(a[a.index("-u") + 1]))
    with kc:
        d = _own_dict(kc)
        seqs = [s for s in _seqs_of(path) if s]
        reads_ = [b"".join(seqs)[i:i + 150] for i in range(0, 30000, 150)]
        reads_ = [_plant(r, [70]) if i % 3 == 0 else r for i, r in enumerate(reads_)]
        text, off = ka.pack_sequences(reads_)
        want = correct_model.correct(text, off, k, d, 2)
        assert sum(x["corrected"] for x in want[1]) >= 10
        assert _host(kc, text, off, 2) == want
        with ka.KmerCounter(ka.Config(k=k, mode=mode, table_slots=1 << 20, min_abundance=1)) as dst:
            dst.table_op(kc, kc, ka.OP_INTERSECT_MIN)
            assert _own_dict(dst) == d
            assert _host(dst, text, off, 2) == want


def test_states_arguments_and_nothing_changes(reads, oracle):
    k = 31
    path, seqs = reads(k)
    d = oracle(path, k)
    kc, st = ka.count_file(path, k, mode=2, min_abundance=1, table_slots=1 << 20)
    with kc:
        text, off = _mixed_text(seqs, 3, n_counted=60)
        before, digest = kc.finish(), kc.output_digest()
        want = correct_model.correct(text, off, k, d, 2)
        assert _host(kc, text, off, 2) == want
        assert _device(kc, text, off, 2) == want
        assert kc.finish() == before == st and kc.output_digest() == digest  # the table is only read
        out = ctypes.create_string_buffer(200)
        t100 = b"ACGT" * 25

        def call(offsets, n_bytes=100, text=t100, out=out):
            o = np.array(offsets, dtype=np.uint64)
            return kc.lib.kc_correct(kc._ctx, text, n_bytes, o.ctypes.data, len(o) - 1, 1, out, None)

        assert call([0, 50, 40, 100]) == KC_ERR_ARG          # decreasing
        assert call([0, 50, 101]) == KC_ERR_ARG              # past n_bytes
        assert call([0, 50, 100], n_bytes=99) == KC_ERR_ARG
        assert call([0, 50, 100], text=None) == KC_ERR_ARG
        assert call([0, 50, 100], out=None) == KC_ERR_ARG
        assert kc.lib.kc_correct(kc._ctx, t100, 100, None, 2, 1, out, None) == KC_ERR_ARG
        assert out.raw == b"\0" * 200
        assert call([0, 50, 50, 100]) == 0 and out.raw[:100] == t100
        assert call([7]) == 0                                # n_seqs = 0: the text is copied
        assert kc.lib.kc_correct(kc._ctx, None, 0, None, 0, 1, None, None) == 0
        assert kc.lib.kc_correct_device(kc._ctx, None, 0, None, 0, 1, None, None, None) == 0
        assert kc.correct([])[0] == [] and len(kc.correct([])[1]) == 0
        # an emptied table: out == text, every base position with covering windows a candidate
        for wipe in (kc.clear_table, kc.reset):
            wipe()
            got = _host(kc, text, off, 1)
            assert got == correct_model.correct(text, off, k, {}, 1)
            assert got[0] == text and sum(x["candidates"] for x in got[1]) > 10000


# ---- 8. the device form on a side stream ----------------------------------------------------------
def test_device_form_on_a_side_stream(reads, counted):
    """On a non-default torch stream, directly after the copy kernels that produce the text there, no
    synchronisation in between."""
    import torch
    k = 31
    kc, d = counted(k)
    text, off = _mixed_text(reads(k)[1], 11)
    want = correct_model.correct(text, off, k, d, 3)
    src = torch.frombuffer(bytearray(text), dtype=torch.uint8).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        staged = torch.empty(len(text), dtype=torch.uint8, device="cuda")
        staged.copy_(src, non_blocking=True)
        dt = staged.flip(0).flip(0)  # a kernel on the stream produces the text
        out = torch.zeros(len(text), dtype=torch.uint8, device="cuda")
        ds = torch.zeros((len(off) - 1) * 16, dtype=torch.uint8, device="cuda")
        kc.correct_device(dt.data_ptr(), len(text), off, out.data_ptr(), 3, ds.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    assert out.cpu().numpy().tobytes() == want[0]
    assert _rows(ds.cpu().numpy().view(ka.CORRECT_STAT_DTYPE)) == want[1]
