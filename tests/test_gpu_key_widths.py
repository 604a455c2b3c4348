"""GPU: every kernel family at every key width (key_widths.py: W = 1 .. 15, the wide end K_HI[W] and
the narrow end K_LO[W] of each), on one input per k that is counted twice: on a roomy table (2^18
slots) and on a full one (table_slots = the distinct count, so that probes run over several buckets
and use the later slots of a bucket).

Expected values never come from the code under test: the C oracle's ``-a 1`` output is the table
({canonical k-mer: T(c)}), the dump of both tables has to equal it, and the pure-Python models
(graph_model, unitig_model, tableop_model, seq_model, correct_model) are applied to it.  All
comparisons are exact.  The counters, the oracle's dictionary and the models' results are made once
per k (and range) and shared by every test below; every case checks on the model that its input
holds what it claims to exercise."""
import subprocess

import numpy as np
import pytest

import correct_model
import graph_model as m
import kaarme_amd as ka
import key_widths as kw
import seq_model
import tableop_model as tm
import unitig_model as um
from conftest import GEN, oracle_count
from seq_model import NO_KMER
from test_gpu_correct import COMP, _host as correct_host, _plant
from test_gpu_graph import RANGES, check_graph, count, same, table_of
from test_gpu_query import _absent, _canonical_expect, _revcomp_keys
from test_gpu_seq import _mixed_text, _stats_rows
from test_gpu_tableop import as_dict, check as check_table_op, empty
from test_gpu_unitig import check_unitigs, claims

pytestmark = pytest.mark.gpu

TABLES = ("roomy", "full")
SENT = 0x5EA7BEEF
MIN_TABLE_SLOTS = 4096  # the smallest table the engine makes (one region)


# ---- what the tests of one k share -----------------------------------------------------------------
def sequences_of(data):
    return [ln for ln in data.split(b"\n") if ln and not ln.startswith(b">")]


def table_op_b_input(k):
    """the second operand's reads: the later half of width_input(k), so that the operands share
    k-mers and the first holds some of its own, and 50 reads of another genome, which only b holds"""
    lines = kw.width_input(k).split(b"\n")
    return b"\n".join(lines[len(lines) // 4 * 2:-1] + kw.width_input(k, other=1000).split(b"\n")[:100]) + b"\n"


def correct_input(seqs, k):
    """(sequences, the indices of the ones with two planted errors five bases apart): reads as they
    are, the last ones of the input (seen once in the 600-base inputs: their errors are weak),
    twenty with one planted error and ten with two"""
    rng = np.random.default_rng(7000 + k)
    L = len(seqs[0])
    single = [_plant(s, [int(p)]) for s, p in zip(seqs[40:60], rng.integers(0, L, 20))]
    double = [_plant(s, [int(p), int(p) + 5]) for s, p in zip(seqs[60:70], rng.integers(0, L - 5, 10))]
    parts = seqs[:10] + seqs[-30:] + single + double
    return parts, range(len(parts) - 10, len(parts))


def seq_stat_input(seqs, k):
    """no, no, one and two windows; forty reads (the wave form); 2048 and 2049 bytes of joined reads
    (the two sides of the workgroup form's threshold) and all of them; all N"""
    r = seqs[0]
    L = len(r)
    joined = b"".join(seqs[50:50 + 2600 // L + 1])
    assert len(joined) > 2049 and L >= k + 1
    return [b"", r[:k - 1], r[:k], r[:k + 1]] + seqs[10:50] + [joined[:2048], joined[:2049], joined, b"N" * 200]


class Width:
    """one k: the input, its two counters, the oracle's dictionary, and the models' results"""

    def __init__(self, k, work):
        self.k, self.W = k, ka.words_for_k(k)
        self.data = kw.width_input(k)
        self.seqs = sequences_of(self.data)
        fa, out = work / f"w{k}.fasta", work / f"w{k}.txt"
        fa.write_bytes(self.data)
        oracle_count(str(fa), k, ["-m", "2", "-a", "1"], out)
        self.d = seq_model.oracle_dict(out)                      # {k-mer bytes: T(c)}: seq_model, correct_model
        self.table = {s.decode(): c for s, c in self.d.items()}  # {k-mer string: T(c)}: graph_model, unitig_model
        self.strings = sorted(self.table)
        self.counts = np.array([self.table[s] for s in self.strings], dtype=np.uint32)
        self.keys = ka.encode_kmers(self.strings, k)
        self.by_key = {tuple(r): int(c) for r, c in zip(self.keys.tolist(), self.counts)}
        self.distinct = len(self.table)
        self.roomy = count(self.data, k)
        self.full = count(self.data, k, table_slots=self.distinct)
        self._graphs, self._units, self._pair = {}, {}, None

    def kc(self, which):
        return self.roomy if which == "roomy" else self.full

    def graph(self, lo, hi):
        if (lo, hi) not in self._graphs:
            self._graphs[lo, hi] = m.graph(self.table, lo, hi)
        return self._graphs[lo, hi]

    def units(self, lo, hi):
        if (lo, hi) not in self._units:
            self._units[lo, hi] = um.unitigs(self.table, lo, hi)
        return self._units[lo, hi]

    def pair(self):
        """(b's counter on a full table of its own, a's dict, b's dict, a result context)"""
        if self._pair is None:
            fb = table_op_b_input(self.k)
            with count(fb, self.k) as sized:
                n_b = sized.finish()["distinct"]
            b = count(fb, self.k, table_slots=n_b)
            self._pair = (b, as_dict(self.full), as_dict(b), empty(self.k))
        return self._pair

    def close(self):
        for kc in (self.roomy, self.full) + (self._pair[::3] if self._pair else ()):
            kc.close()


@pytest.fixture(scope="module")
def widths(tmp_path_factory):
    """k -> its Width, made once"""
    work = tmp_path_factory.mktemp("key_widths")
    made = {}

    def get(k):
        if k not in made:
            made[k] = Width(k, work)
        return made[k]

    yield get
    for w in made.values():
        w.close()


# ---- 1. counting: the dump of both tables is the oracle's output --------------------------------------
@pytest.mark.parametrize("k", kw.CHEAP_KS)
def test_count_and_dump(k, widths):
    w = widths(k)
    assert w.distinct > 500 and w.counts.max() >= 2
    for which in TABLES:
        ok = same(table_of(w.kc(which)), w.table)
        assert ok, which
    roomy, full = w.roomy.finish(), w.full.finish()
    assert roomy["distinct"] == full["distinct"] == w.distinct
    assert w.counts.max() < 16383 and roomy["windows"] == full["windows"] == int(w.counts.sum())  # (none saturates)
    assert roomy["table_slots"] >= 1 << 18 > 3 * w.distinct
    print(f"k={k} W={w.W} distinct={w.distinct} full table_slots={full['table_slots']}")
    if w.distinct >= MIN_TABLE_SLOTS:
        assert full["table_slots"] < 2 * w.distinct
    else:  # all 512 canonical 5-mers: the smallest table there is
        assert k == 5 and w.distinct == 512 and full["table_slots"] == MIN_TABLE_SLOTS


# ---- 2. the cheap families ----------------------------------------------------------------------------
@pytest.mark.parametrize("which", TABLES)
@pytest.mark.parametrize("k", kw.CHEAP_KS)
def test_lookup(k, which, widths):
    """both strands of every key, random and one-base-off keys (absent, mostly), a bit above the
    k-mer, and a device call of a length that is no multiple of anything between sentinels"""
    import torch
    w, kc = widths(k), widths(k).kc(which)
    got = kc.lookup(w.keys)
    assert got.dtype == np.uint32 and (got == w.counts).all()
    assert (kc.lookup(_revcomp_keys(w.keys, k)) == w.counts).all()
    absent = _absent(None, k, 2000, 7000 + k)
    want_absent = _canonical_expect(w.by_key, absent, k)
    assert k < 16 or (want_absent == 0).sum() > 1900
    assert (kc.lookup(absent) == want_absent).all()
    near = w.keys[:2000].copy()
    near[:, -1] ^= np.uint64(2)
    assert (kc.lookup(near) == _canonical_expect(w.by_key, near, k)).all()
    bad = w.keys[:50].copy()
    bad[:, w.W - 1 - (2 * k) // 64] |= np.uint64(1) << np.uint64((2 * k) % 64)  # a bit at position 2k: no k-mer
    assert not kc.lookup(bad).any()
    mixed = np.ascontiguousarray(np.concatenate([w.keys[:600], absent[:401]]))
    n = len(mixed)
    dk = torch.from_numpy(mixed.view(np.int64)).cuda()
    out = torch.full((n + 32,), SENT, dtype=torch.int32, device="cuda")
    kc.lookup_device(dk.data_ptr(), n, out.data_ptr() + 16 * 4)
    torch.cuda.synchronize()
    res = out.cpu().numpy()
    assert n % 64 and (res[:16] == SENT).all() and (res[16 + n:] == SENT).all()
    assert (res[16:16 + n].view(np.uint32) == np.concatenate([w.counts[:600], want_absent[:401]])).all()


@pytest.mark.parametrize("k", kw.CHEAP_KS)
def test_histogram(k, widths):
    w = widths(k)
    want = np.bincount(np.minimum(w.counts.astype(np.int64), 16384), minlength=16385)
    assert (want > 0).sum() >= 3
    for which in TABLES:
        h = w.kc(which).histogram(16385)
        assert h.dtype == np.uint64 and (h == want).all(), which
        assert (w.kc(which).histogram(4) == np.bincount(np.minimum(w.counts.astype(np.int64), 3), minlength=4)).all()


@pytest.mark.parametrize("k", kw.CHEAP_KS)
def test_text_counts(k, widths):
    w = widths(k)
    text = _mixed_text(w.seqs, k, 7000 + k)  # (not the seed of the input: its random reads would repeat the genome)
    want = np.array(seq_model.text_counts(text, k, w.d), dtype=np.uint32)
    valid = want != NO_KMER
    assert valid.sum() > 1000 and (want[valid] > 0).sum() > 1000 and (~valid).sum() > 1000
    assert k < 16 or (want[valid] == 0).sum() > 1000  # (every 5-mer is in the table)
    for which in TABLES:
        got = w.kc(which).text_counts(text)
        assert got.dtype == np.uint32 and got.shape == (len(text),)
        assert (got == want).all(), which
    # the other strand: the window at p is the window at n - p - k of the reverse complement
    back = w.roomy.text_counts(text.translate(COMP)[::-1])
    assert (back[back != NO_KMER] == want[valid][::-1]).all()


@pytest.mark.parametrize("k", kw.CHEAP_KS)
def test_seq_stats(k, widths):
    w = widths(k)
    seqs = seq_stat_input(w.seqs, k)
    text, off = ka.pack_sequences(seqs)
    for solid_min in (1, 2):
        want = seq_model.seq_stats(text, off, k, w.d, solid_min)
        assert [x["windows"] for x in want[:4]] == [0, 0, 1, 2] and want[-1]["windows"] == 0
        assert all(x["windows"] == len(s) - k + 1 and x["present"] > 0 for x, s in zip(want[4:-1], seqs[4:-1]))
        assert want[-2]["windows"] > 2049 - k and (k < 16 or want[-2]["present"] < want[-2]["windows"])  # the joints' k-mers are absent
        for which in TABLES:
            got = w.kc(which).seq_stats(seqs, solid_min=solid_min)
            assert got.dtype == ka.SEQ_STAT_DTYPE and _stats_rows(got) == want, (which, solid_min)


@pytest.mark.parametrize("k", kw.CHEAP_KS)
def test_compact(k, widths):
    """the compact representation built from either table gives every k-mer back with its count, by
    reconstruction and by key"""
    w = widths(k)
    flipped = w.keys[:500].copy()
    flipped[:, -1] ^= np.uint64(1)  # the last character's low bit
    want_flipped = np.array([w.by_key.get(tuple(r), 0) for r in flipped.tolist()], dtype=np.uint32)
    for which in TABLES:
        kc = w.kc(which)
        info = kc.compact()
        assert info["kmers"] == w.distinct
        recs, max_hops, _ = kc.compact_dump()
        assert max_hops <= max(0, k - 2)
        ok = same(dict(ka.decode_records(recs, k)), w.table)
        assert ok, which
        assert (kc.compact_lookup(w.keys) == w.counts).all(), which
        assert (kc.compact_lookup(flipped) == want_flipped).all(), which


# ---- 3. the model-heavy families --------------------------------------------------------------------------
def neighbor_input(w):
    """(1000 held k-mers, them + their other strands + 300 k-mers one base off a held one, the model's
    answers): the last are absent; off at the first or the last base (100 each), they keep the held
    k-mer's neighbours on the other side, off at a random base they have none"""
    rng = np.random.default_rng(7000 + w.k)
    held = [w.strings[i] for i in rng.choice(len(w.strings), 1000, replace=False)]
    at = [0] * 100 + [w.k - 1] * 100 + rng.integers(0, w.k, 100).tolist()
    off = [c[:j] + "ACGT"[("ACGT".index(c[j]) + 1) % 4] + c[j + 1:] for c, j in zip(held[:300], at)]
    strings = held + [m.rc(c) for c in held] + off
    want = np.array([m.neighbors(w.table, x) for x in strings], dtype=np.uint32)
    assert want[:1000].any(axis=1).sum() > 900 and sum(x in w.table or m.rc(x) in w.table for x in off) < 30
    assert want[2000:2200].any(axis=1).sum() > 150 and (want[2200:] == 0).all(axis=1).sum() > 50
    return held, strings, want


@pytest.mark.parametrize("which", TABLES)
@pytest.mark.parametrize("k", kw.HEAVY_NEW_KS)
def test_neighbors(k, which, widths):
    w, kc = widths(k), widths(k).kc(which)
    held, strings, want = neighbor_input(w)
    got = kc.neighbors(ka.encode_kmers(strings, k))
    assert got.shape == (len(strings), 8) and got.dtype == np.uint32
    assert (got == want).all()
    assert (got[1000:2000][:, ::-1] == got[:1000]).all()  # the other strand: R and L swap and complement
    bad = ka.encode_kmers(held[:8], k)
    bad[:, w.W - 1 - (2 * k) // 64] |= np.uint64(1) << np.uint64((2 * k) % 64)
    assert got[:8].any() and not kc.neighbors(bad).any()


def input_claims(w, lo, hi):
    """what the graph and unitig cases exercise, on the model: more than 100 unitigs, one of 50 nodes
    and more, one of one node; dead ends, forks and links; a range that leaves nodes out"""
    units = w.units(lo, hi)
    st = um.stats(units, w.k)
    claims(units)
    assert st["nodes"] > st["unitigs"] > 1
    assert (lo, hi) == (1, 0) or st["nodes"] < len(w.table)
    _, gst = w.graph(lo, hi)
    sd = gst["side_degree"]
    assert sd[0] > 0 and sd[2] + sd[3] + sd[4] > 0 and gst["link_ends"] > 100 and gst["nodes"] == st["nodes"]


@pytest.mark.parametrize("which", TABLES)
@pytest.mark.parametrize("lo,hi", RANGES)
@pytest.mark.parametrize("k", kw.HEAVY_NEW_KS)
def test_graph(k, lo, hi, which, widths):
    w = widths(k)
    input_claims(w, lo, hi)
    check_graph(w.kc(which), w.table, lo, hi, want=w.graph(lo, hi))


@pytest.mark.parametrize("which", TABLES)
@pytest.mark.parametrize("lo,hi", RANGES)
@pytest.mark.parametrize("k", kw.HEAVY_NEW_KS)
def test_unitigs(k, lo, hi, which, widths):
    w = widths(k)
    input_claims(w, lo, hi)
    check_unitigs(w.kc(which), w.table, lo, hi, want=w.units(lo, hi))


@pytest.mark.parametrize("op", tm.OPS, ids=tm.OP_NAMES)
@pytest.mark.parametrize("k", kw.HEAVY_NEW_KS)
def test_table_op(k, op, widths):
    """a = the full table (swept), b = another input's full table (probed, and swept by the unions),
    the result in a roomy one"""
    w = widths(k)
    b, da, db, dst = w.pair()
    assert len(da) == w.distinct and b.finish()["table_slots"] < 2 * len(db) and dst.finish()["table_slots"] >= 1 << 18
    assert set(da) & set(db) and set(da) - set(db) and set(db) - set(da)
    dst.reset()
    st = dst.table_op(w.full, b, op)
    check_table_op(dst, da, db, op, st)
    assert dst.finish()["inserted"] == st["out_sum"]


@pytest.mark.parametrize("k", kw.HEAVY_NEW_KS)
def test_correct(k, widths):
    w = widths(k)
    seqs, double = correct_input(w.seqs, k)
    text, off = ka.pack_sequences(seqs)
    want, wstats = correct_model.correct(text, off, k, w.d, 2)
    assert sum(s["corrected"] for s in wstats) == sum(a != b for a, b in zip(want, text)) >= 1
    left = [i for i in double if wstats[i]["candidates"] > 0 and want[int(off[i]):int(off[i + 1])] == text[int(off[i]):int(off[i + 1])]]
    assert left  # an erroneous read that the rule leaves alone
    for which in TABLES:
        assert correct_host(w.kc(which), text, off, 2) == (want, wstats), which
    # the other strand: the reverse complement corrects to the reverse complement of the output
    n = len(text)
    back, bstats = correct_host(w.roomy, text.translate(COMP)[::-1], (n - off.astype(np.int64))[::-1], 2)
    assert back == want.translate(COMP)[::-1] and bstats == wstats[::-1]


# ---- 4. the distinct-count sketch of keys of five words and more ------------------------------------------
@pytest.fixture(scope="module")
def long_reads(tmp_path_factory):
    """4000 reads of 600 bases over a 400 kbp genome, as a host image and a device image"""
    import torch
    fa = tmp_path_factory.mktemp("key_widths_hll") / "r.fasta"
    subprocess.run([GEN, str(fa), "4000", "600", "400000", "-s", "11", "-n", "0.002"], check=True)
    data = open(fa, "rb").read()
    return data, torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()


@pytest.mark.parametrize("k", kw.HLL_KS)
def test_estimate_distinct_unsampled(k, long_reads):
    """kc_estimate_distinct_device past four words hashes every distinct k-mer (k_hll<W>; up to four
    words a sample, test_gpu_parity.py test_distinct_estimate): 2^14 registers, ~0.8 % standard
    error, against the exact distinct count of the same image and of its first chunk"""
    data, img = long_reads
    chunks = ka.plan_chunks(data, k, ka.FMT_FASTA, 1 << 20)
    assert len(chunks) >= 3
    cfg = ka.Config(k=k, mode=2, min_abundance=1, table_slots=1 << 22)
    with ka.KmerCounter(cfg) as kc:
        est = kc.estimate_distinct_device(img.data_ptr(), chunks, ka.FMT_FASTA)
        est_small = kc.estimate_distinct_device(img.data_ptr(), chunks[:1], ka.FMT_FASTA)
        assert kc.finish()["distinct"] == 0  # it counts nothing
        kc.count_device(img.data_ptr(), chunks, ka.FMT_FASTA)
        st = kc.finish()
        exact = st["distinct"]
    with ka.KmerCounter(cfg) as kc:
        kc.count_device(img.data_ptr(), chunks[:1], ka.FMT_FASTA)
        exact_small = kc.finish()["distinct"]
    print(f"k={k} estimate {est:.0f} of {exact}, first chunk {est_small:.0f} of {exact_small}")
    assert st["windows"] > exact > exact_small > 50000  # (three times the registers and more)
    assert abs(est - exact) / exact < 0.04, (est, exact)
    assert abs(est_small - exact_small) / exact_small < 0.04, (est_small, exact_small)
