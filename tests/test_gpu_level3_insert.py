"""Level 3's insert (kc_count_impl.h k_p3 insert_one) on keys built for it: probe chains, the wrap from
bucket 511 to bucket 0, one tag among several keys of a bucket, a hot key's claim race and adds, and a
region one key too full.

Every read of an input is exactly one chosen k-mer, so the input's dictionary {k-mer: reads} is the
expected result, independent of the code under test.  A key is built backwards from word 0 of its
table key (kc_common.h to_tkey): x, the top 32 bits, picks the region (x R >> 32) and the start
bucket (the top 9 bits of x R mod 2^32); the low byte picks the slot tag.  tmix is inverted
(y = t ^ (t >> 32), times TMUL^-1), one-word keys keep what stays below 4^k after ^ MIX_C, wider keys
set their last word to x ^ the side hash of the others; bloom_model.table_key0 then confirms word 0 of
every k-mer built.  The table's R is read back from the job's stats.

Tables: one-word keys in exactly 2^16 regions (6-byte level-2 records, the start bucket from the record)
and in a table asked for 3 regions; two-word keys the same (12-byte records against the region).  The
geometry is F1 x F2 with F2 a power of two, so 3 regions asked for are 4 held."""
import random

import pytest

import bloom_model as bm
import kaarme_amd as ka

pytestmark = pytest.mark.gpu

M64 = (1 << 64) - 1
MIX_C = 0x9E3779B97F4A7C15
TMUL_INV = 0xF1DE83E19937733D
BPR = 512
KC_ERR_TABLE_FULL = -3


def _S(k):
    return 16 // (k // 32 + 2)  # BUCKET_WORDS / (W + 1)


def _small_slots(k):
    """asks for 3 regions: 1.25 x slots in (1024 S, 1536 S]"""
    return 1024 * _S(k)


BIG = {31: 200_000_000, 51: 134_217_000}  # 2^16 regions each (k = 31: 61 036 asked, rounded up for the records)


def _regions(k, slots):
    if slots in BIG.values():
        return 1 << 16
    return 4


def _kmer_of(words, k):
    v = 0
    for w in words:
        v = (v << 64) | w
    return "".join("ACGT"[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


def _tmix_inv(t):
    return ((t ^ (t >> 32)) * TMUL_INV) & M64


class Keys:
    """distinct k-mers with a chosen region, start bucket and tag"""

    def __init__(self, k, R, seed):
        self.k, self.R, self.W = k, R, k // 32 + 1
        self.rng = random.Random(seed)
        self.seen = set()

    def _x(self, region, bucket):
        R = self.R
        if bucket is None:
            lo, hi = -(-(region << 32) // R), -(-((region + 1) << 32) // R)
        else:
            lo = -(-((region << 32) + (bucket << 23)) // R)
            hi = -(-((region << 32) + ((bucket + 1) << 23)) // R)
        assert lo < hi
        return self.rng.randrange(lo, hi)

    def one(self, region, bucket=None, tag_byte=None):
        k, W = self.k, self.W
        top = 2 * k - 64 * (W - 1)
        for _ in range(100000):
            x = self._x(region, bucket)
            b0 = self.rng.randrange(1, 256) if tag_byte is None else tag_byte
            t0 = (x << 32) | (self.rng.randrange(1 << 24) << 8) | b0
            y = _tmix_inv(t0)
            if W == 1:
                words = [y ^ MIX_C]
                if words[0] >> (2 * k):
                    continue
            else:
                if y == 0:
                    continue
                words = [self.rng.randrange(1 << top)] + [self.rng.randrange(1 << 64) for _ in range(W - 2)]
                g = 0
                for i, w in enumerate(words):
                    g = bm.fmix64(g ^ w ^ ((0x243F6A8885A308D3 * (i + 1)) & M64))
                words.append(y ^ g)
            s = _kmer_of(words, k)
            if s in self.seen or bm.canonical_words(s) != words:  # (the other strand is the canonical one)
                continue
            assert bm.table_key0(s) == t0
            assert (x * self.R) >> 32 == region
            assert bucket is None or ((x * self.R) & 0xFFFFFFFF) >> 23 == bucket
            self.seen.add(s)
            return s
        raise AssertionError("no key found")

    def many(self, n, region, bucket=None, tag_byte=None):
        return [self.one(region, bucket, tag_byte) for _ in range(n)]


def _count(path, k, slots):
    image = open(path, "rb").read()
    chunks = ka.plan_chunks(image, k, ka.FMT_FASTA, 0)
    staged = 4096 + sum((ln + 4095) // 4096 * 4096 for _, ln, _ in chunks)
    with ka.KmerCounter(ka.Config(k=k, mode=2, min_abundance=1, table_slots=slots, batch_bytes=staged)) as kc:
        for off, ln, bh in chunks:
            kc.count_chunk(image[off:off + ln], ka.FMT_FASTA, bool(bh))
        st = kc.finish()
        return kc.lines(), st


def _run(reads, k, slots, tmp_path, monkeypatch):
    """counts `reads` on the partitioned path, checks the dictionary and the direct path's answer"""
    path = tmp_path / "reads.fasta"
    path.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(reads)))
    want = {}
    for s in reads:
        want[s] = want.get(s, 0) + 1
    want_lines = sorted(f"{s} {c}" for s, c in want.items())
    monkeypatch.setenv("KC_INSERT_PATH", "partitioned")
    lines, st = _count(str(path), k, slots)
    assert st["table_slots"] == _regions(k, slots) * BPR * _S(k), st["table_slots"]
    assert st["windows"] == len(reads) and st["heavy_records"] == 0
    assert lines == want_lines
    assert st["distinct"] == len(want)
    monkeypatch.setenv("KC_INSERT_PATH", "direct")
    lines_d, st_d = _count(str(path), k, slots)
    assert lines_d == lines and st_d["distinct"] == st["distinct"]


def _shuffled_with_multiplicities(keys, rng):
    reads = [s for i, s in enumerate(keys) for _ in range(1 + i % 5)]  # multiplicities 1..5
    rng.shuffle(reads)
    return reads


TABLES = [(31, BIG[31]), (31, _small_slots(31)), (51, _small_slots(51)), (51, BIG[51])]
WIDE = [(k, _small_slots(k)) for k in (95, 127, 223, 479)]  # S = 4, 3, 2, 1


@pytest.mark.parametrize("bucket", [200, BPR - 1], ids=["chain", "wrap"])
@pytest.mark.parametrize("k,slots", TABLES + WIDE)
def test_probe_chain(k, slots, bucket, tmp_path, monkeypatch):
    """3 S + 2 keys of one start bucket: three full buckets and two slots of a fourth; from bucket 511
    the chain wraps to bucket 0"""
    R = _regions(k, slots)
    gen = Keys(k, R, seed=k + bucket)
    keys = gen.many(3 * _S(k) + 2, region=R - 1 if bucket == 200 else 1, bucket=bucket)
    _run(_shuffled_with_multiplicities(keys, gen.rng), k, slots, tmp_path, monkeypatch)


@pytest.mark.parametrize("k,slots", TABLES)
def test_one_tag_among_others(k, slots, tmp_path, monkeypatch):
    """a bucket's keys with one tag (S / 2 + 1 of them, each a candidate of the others' probes) among
    keys with other tags, S + 2 keys in all"""
    R, S = _regions(k, slots), _S(k)
    gen = Keys(k, R, seed=7 * k)
    same = gen.many(S // 2 + 1, region=2, bucket=77, tag_byte=0x5A)
    others = [gen.one(2, 77, tag_byte=t) for t in (0x5B, 0x01, 0x80, 0xFF, 0x5A ^ 0x80, 0x2D)[:S + 2 - len(same)]]
    keys = [s for pair in zip(same, others) for s in pair] + same[len(others):] + others[len(same):]
    assert len(set(keys)) == S + 2
    _run(_shuffled_with_multiplicities(keys, gen.rng), k, slots, tmp_path, monkeypatch)


@pytest.mark.parametrize("k,slots", TABLES)
def test_hot_key(k, slots, tmp_path, monkeypatch):
    """one key 5 000 times between the reads of 2 000 other keys of its region, never next to itself
    (a read is one window, so level 1's heavy table sees no repeat): the claim race and the adds"""
    R = _regions(k, slots)
    gen = Keys(k, R, seed=11 * k)
    hot = gen.one(region=3)
    others = gen.many(2000, region=3)
    reads = []
    for i in range(5000):
        reads += [hot, others[i % 2000]]
    _run(reads, k, slots, tmp_path, monkeypatch)


@pytest.mark.parametrize("k,slots", TABLES)
def test_region_one_key_too_full(k, slots, tmp_path, monkeypatch):
    """512 S + 1 distinct keys of one region: finish() returns the table-full error"""
    R = _regions(k, slots)
    gen = Keys(k, R, seed=13 * k)
    reads = gen.many(BPR * _S(k) + 1, region=R // 2)
    path = tmp_path / "reads.fasta"
    path.write_text("".join(f">r{i}\n{s}\n" for i, s in enumerate(reads)))
    monkeypatch.setenv("KC_INSERT_PATH", "partitioned")
    with pytest.raises(ka.KcError) as e:
        _count(str(path), k, slots)
    assert e.value.code == KC_ERR_TABLE_FULL


@pytest.mark.parametrize("k,slots", TABLES)
def test_direct_batch_on_a_partitioned_table(k, slots, tmp_path, monkeypatch):
    """the same reads twice into one table, first on the partitioned path, then on the direct one, which
    probes from bucket_in_region: a key that level 3 had put on a chain from another start bucket would
    be claimed a second time and listed twice instead of once with both passes' reads"""
    import torch
    R = _regions(k, slots)
    gen = Keys(k, R, seed=17 * k)
    keys = gen.many(3 * _S(k) + 2, region=R - 1, bucket=BPR - 1) + gen.many(300, region=R - 1) + gen.many(300, region=0)
    reads = _shuffled_with_multiplicities(keys, gen.rng)
    host = "".join(f">r{i}\n{s}\n" for i, s in enumerate(reads)).encode()
    img = torch.frombuffer(bytearray(host), dtype=torch.uint8).cuda()
    chunks = ka.plan_chunks(host, k, ka.FMT_FASTA, 0)
    want = {}
    for s in reads:
        want[s] = want.get(s, 0) + 2
    with ka.KmerCounter(ka.Config(k=k, mode=2, min_abundance=1, table_slots=slots, batch_bytes=len(host) + 8192)) as kc:
        monkeypatch.setenv("KC_INSERT_PATH", "partitioned")
        kc.count_device(img.data_ptr(), chunks, ka.FMT_FASTA)
        torch.cuda.synchronize()
        monkeypatch.setenv("KC_INSERT_PATH", "direct")
        kc.count_device(img.data_ptr(), chunks, ka.FMT_FASTA)
        st = kc.finish()
        assert st["windows"] == 2 * len(reads) and st["distinct"] == len(want)
        assert kc.lines() == sorted(f"{s} {c}" for s, c in want.items())
