"""GPU: the de Bruijn graph of the counted table (kc_neighbors*, kc_graph*; KmerCounter.neighbors /
graph / graph_stats and their *_device forms) against the pure-Python model graph_model.py applied
to the table's own dump().

Inputs are generated here.  Expected = the model on decode_records(dump()); actual = the records as
a {k-mer: (T(c), flags)} dict and the returned statistics, compared exactly."""
import ctypes

import numpy as np
import pytest

import graph_model as m
import kaarme_amd as ka

pytestmark = pytest.mark.gpu

KC_ERR_ARG, KC_ERR_STATE = -1, -4
KS = [15, 31, 32, 63, 65, 479]  # W = 1 (8 slots), 1, 2, 2, 3, 15 (one slot per bucket)
RANGES = [(1, 0), (2, 0), (2, 50)]
STAT_WORDS = 10


# ---- inputs and helpers --------------------------------------------------------------------------
def _bases(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _reads(rng, genome, n, length, err=0.0):
    """n reads of `length` bases from random places of the genome, each base substituted with
    probability err"""
    out = []
    for i, s in enumerate(rng.integers(0, len(genome) - length + 1, n)):
        r = bytearray(genome[s:s + length])
        for p in np.flatnonzero(rng.random(length) < err):
            r[p] = b"ACGT"[(b"ACGT".index(r[p]) + int(rng.integers(1, 4))) % 4]
        out.append(b">r%d\n%s\n" % (i, bytes(r)))
    return b"".join(out)


def make_reads(seed, n_reads=2000, read_len=100, genome_len=40000, rep_len=300, err=0.01):
    """reads with 1 % substitutions from a random genome that holds a 300-base repeat three times"""
    rng = np.random.default_rng(seed)
    g = bytearray(_bases(rng, genome_len))
    rep = _bases(rng, rep_len)
    for at in (genome_len // 8, genome_len // 2, genome_len - genome_len // 5):
        g[at:at + rep_len] = rep
    return _reads(rng, bytes(g), n_reads, read_len, err=err)


def count(data, k, bloom=False, **cfg):
    """a finished counter of the FASTA bytes (host chunks)"""
    chunks = ka.plan_chunks(data, k, ka.FMT_FASTA)
    cfg.setdefault("mode", 2)
    cfg.setdefault("table_slots", 1 << 18)
    cfg.setdefault("batch_bytes", len(data) + 4096 * (len(chunks) + 2))
    kc = ka.KmerCounter(ka.Config(k=k, min_abundance=1, bf_enable=bloom, **cfg))
    mv = memoryview(data)
    if bloom:
        for off, ln, bh in chunks:
            kc.bloom_chunk(bytes(mv[off:off + ln]), ka.FMT_FASTA, bool(bh))
        kc.bloom_finalize()
    for off, ln, bh in chunks:
        kc.count_chunk(bytes(mv[off:off + ln]), ka.FMT_FASTA, bool(bh))
    kc.finish()
    return kc


def table_of(kc):
    """{canonical k-mer: T(c)} of dump()"""
    return dict(ka.decode_records(kc.dump(), kc.cfg.k))


def records_dict(records, k):
    """{k-mer: (T(c), flags)} of graph records; the bits above the 16 flag bits are 0"""
    assert not (records[:, -1] >> np.uint64(48)).any()
    out = {s: (v & 0xFFFFFFFF, v >> 32) for s, v in ka.decode_records(records, k)}
    assert len(out) == len(records)
    return out


def same(got, want):
    """got == want for two big dicts, with a short account of the difference"""
    if got == want:
        return True
    bad = [key for key in set(got) | set(want) if got.get(key) != want.get(key)]
    print(f"{len(got)} records against {len(want)} expected, {len(bad)} differ, e.g. "
          f"{[(key, got.get(key), want.get(key)) for key in sorted(bad)[:5]]}")
    return False


def check_graph(kc, table, lo=1, hi=0, want=None):
    """kc.graph(lo, hi) and kc.graph_stats(lo, hi) == the model on the table; returns the model's"""
    flags, st = want or m.graph(table, lo, hi)
    records, got_st = kc.graph(lo, hi)
    assert got_st == st, (lo, hi, got_st, st)
    ok = same(records_dict(records, kc.cfg.k), {c: (table[c], f) for c, f in flags.items()})
    assert ok, (lo, hi)
    assert kc.graph_stats(lo, hi) == st
    return flags, st


@pytest.fixture(scope="module")
def counted():
    """k -> (counter, its table as a dict, the model's graph per range), made once"""
    made = {}

    def get(k):
        if k not in made:
            data = make_reads(k, 300, 600) if k > 400 else make_reads(k)
            kc = count(data, k)
            made[k] = (kc, table_of(kc), {})
        return made[k]

    yield get
    for kc, _, _ in made.values():
        kc.close()


def model(counted, k, lo=1, hi=0):
    kc, table, graphs = counted(k)
    if (lo, hi) not in graphs:
        graphs[lo, hi] = m.graph(table, lo, hi)
    return graphs[lo, hi]


# ---- 1. every key width ----------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", RANGES)
@pytest.mark.parametrize("k", KS)
def test_every_key_width(k, lo, hi, counted):
    """(k = 479: a window of 479 bases is free of the 1 % substitutions 8 times in 1000 and the
    repeat is shorter than k, so nearly every k-mer is seen once and this input has dead ends and
    links but no fork, and no node at all from T(c) >= 2 on -- test_wide_keys_with_forks covers
    that ground)"""
    kc, table, _ = counted(k)
    flags, st = model(counted, k, lo, hi)
    sd = st["side_degree"]
    if k < 479:
        assert sd[0] > 0 and sd[2] + sd[3] + sd[4] > 0 and st["link_ends"] > 100  # dead ends, forks, links
        assert 1000 < st["nodes"] <= len(table)
    elif lo == 1:
        assert sd[0] > 0 and st["link_ends"] > 100 and st["nodes"] == len(table) > 1000
    check_graph(kc, table, lo, hi, want=(flags, st))


@pytest.mark.parametrize("k", [479, 257])
def test_wide_keys_with_forks(k):
    """fifteen- and nine-word keys on reads whose graph forks in every range: a 600-base repeat
    (longer than k) three times in an 8 kb genome, 1 substitution in 2000 bases"""
    with count(make_reads(k, 300, 600, 8000, rep_len=600, err=0.0005), k) as kc:
        table = table_of(kc)
        for lo, hi in RANGES:
            flags, st = m.graph(table, lo, hi)
            sd = st["side_degree"]
            assert sd[0] > 0 and sd[2] + sd[3] + sd[4] > 0 and st["link_ends"] > 100 and st["nodes"] > 1000
            check_graph(kc, table, lo, hi, want=(flags, st))


# ---- 2. dense small k ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 5, 6])
def test_dense_small_k(k):
    rng = np.random.default_rng(100 + k)
    with count(b">t\n" + _bases(rng, 3000) + b"\n", k, table_slots=1 << 14) as kc:
        table = table_of(kc)
        med = int(np.median(list(table.values())))
        flags, st = m.graph(table, med, 0)
        if k >= 5:
            assert all(st["side_degree"]), st
        if k == 6:
            assert st["palindromes"] > 0
        check_graph(kc, table, med, 0, want=(flags, st))
        check_graph(kc, table)


# ---- 3. special structures -------------------------------------------------------------------------
def test_circle_is_one_closed_unitig():
    k = 31
    rng = np.random.default_rng(7)
    circle = _bases(rng, 500)
    data = _reads(rng, circle * 3, 400, 100)
    with count(data, k, table_slots=1 << 14) as kc:
        table = table_of(kc)
        flags, st = m.graph(table)
        assert st["nodes"] == 500 and st["link_ends"] == 1000 and st["open_unitigs"] == 0
        assert st["side_degree"] == [0, 1000, 0, 0, 0]
        check_graph(kc, table, want=(flags, st))


def test_self_edges_never_link():
    k = 31
    hair = "ACGGTCAATGCCTGAAGTCCATGACCGTTAGACT"  # the read runs on into its own reverse complement
    data = (">a\n" + "A" * 60 + "\n>ca\n" + "CA" * 40 + "\n>h\n" + hair + m.rc(hair) + "\n").encode()
    with count(data, k, table_slots=1 << 14) as kc:
        table = table_of(kc)
        flags, st = m.graph(table)
        assert flags["A" * k] == 0x8011  # follows and precedes itself; no link
        mid = m.canon((hair + m.rc(hair))[len(hair) - 15:len(hair) + 16])  # the hairpin's turn
        assert mid != m.rc(mid) and flags[mid] & 0x300 != 0x300 and bin(flags[mid] & 0xFF).count("1") >= 1
        loops = [c for c in flags if any(m.canon(z) == c for z in m.neighbor_strings(c))]
        assert len(loops) >= 2
        for c in loops:  # a side whose one neighbour is the node itself has no link
            nb = m.edge_info(set(flags), c)[1]
            for s, bit in (("R", m.LINK_R), ("L", m.LINK_L)):
                if len(nb[s]) == 1 and nb[s][0][0] == c:
                    assert not flags[c] & bit
        check_graph(kc, table, want=(flags, st))


# ---- 4. a full table ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [31, 51])
def test_full_table(k):
    """table_slots = the distinct count: probe sequences run over several buckets and wrap"""
    data = make_reads(40 + k)
    with count(data, k, table_slots=1 << 20) as kc0:
        distinct = kc0.finish()["distinct"]
    with count(data, k, table_slots=distinct) as kc:
        st = kc.finish()
        assert st["distinct"] == distinct and st["table_slots"] < 2 * distinct
        table = table_of(kc)
        check_graph(kc, table, 1, 0)
        check_graph(kc, table, 2, 0)
        keys = ka.encode_kmers(list(table)[:4000], k)
        want = np.array([m.neighbors(table, c) for c in list(table)[:4000]], dtype=np.uint32)
        assert (kc.neighbors(keys) == want).all()


# ---- 5. count semantics and states -----------------------------------------------------------------
@pytest.mark.parametrize("mode,n_a,t_a", [(0, 65536 + 2, 2), (2, 20000, 16383)])
def test_the_range_is_on_the_reported_count(mode, n_a, t_a):
    """a poly-A k-mer counted 65538 times reads back 2 in -m 0, one counted 20000 times 16383 in
    -m 2: the node range is on T(c), not on the raw count"""
    k = 31
    rng = np.random.default_rng(11)
    tail = b"C" + _bases(rng, 400)  # (the C ends the run of A's)
    data = b">a\n" + b"A" * (k - 1 + n_a) + tail + b"\n>b\n" + tail + b"\n"
    with count(data, k, mode=mode, table_slots=1 << 14) as kc:
        table = table_of(kc)
        assert table["A" * k] == t_a
        for lo, hi in ((1, 0), (t_a, t_a), (t_a + 1, 0), (1, t_a - 1), (2, 2)):
            flags, _ = check_graph(kc, table, lo, hi)
            assert ("A" * k in flags) == (lo <= t_a and (hi == 0 or t_a <= hi))
        got = kc.neighbors(ka.encode_kmers(["A" * k], k))[0]
        assert got.tolist() == m.neighbors(table, "A" * k) and got[0] == got[4] == t_a


def test_bloom_gated_table():
    k = 31
    data = make_reads(5)
    with count(data, k, bloom=True, est_unique=150000, fpr=0.01) as kc, count(data, k) as plain:
        table = table_of(kc)
        assert 1000 < len(table) < len(table_of(plain))  # the gate dropped k-mers seen once
        check_graph(kc, table)
        check_graph(kc, table, 2, 0)


def test_emptied_table_has_no_nodes(counted):
    k = 31
    data = make_reads(k)
    keys = ka.encode_kmers(list(counted(k)[1])[:100], k)
    zero = {"nodes": 0, "edge_ends": 0, "link_ends": 0, "isolated": 0, "palindromes": 0, "side_degree": [0] * 5,
            "open_unitigs": 0}
    with count(data, k) as kc:
        assert kc.graph_stats()["nodes"] == len(counted(k)[1]) and kc.neighbors(keys).any()
        for empty_it in (kc.clear_table, kc.reset):
            empty_it()
            records, st = kc.graph()
            assert records.shape == (0, 2) and st == zero
            assert not kc.neighbors(keys).any()
            chunks = ka.plan_chunks(data, k, ka.FMT_FASTA)
            for off, ln, bh in chunks:
                kc.count_chunk(data[off:off + ln], ka.FMT_FASTA, bool(bh))
            kc.finish()
            assert kc.graph_stats()["nodes"] == len(counted(k)[1])


def test_argument_and_state_errors(counted):
    kc, table, _ = counted(31)
    lib = kc.lib
    out = np.zeros(32, dtype=np.uint32)
    keys = np.zeros((4, 1), dtype=np.uint64)
    st = ka.kc_graph_stats()
    assert lib.kc_neighbors(kc._ctx, keys.ctypes.data, 4, 2, out.ctypes.data) == KC_ERR_ARG
    assert lib.kc_neighbors(kc._ctx, None, 4, 0, out.ctypes.data) == KC_ERR_ARG
    assert lib.kc_neighbors(kc._ctx, keys.ctypes.data, 4, 0, None) == KC_ERR_ARG
    assert lib.kc_neighbors(kc._ctx, None, 0, 0, None) == 0
    assert lib.kc_neighbors_device(kc._ctx, None, 0, 1, None, None) == 0
    assert lib.kc_neighbors_device(kc._ctx, None, 1, 0, None, None) == KC_ERR_ARG
    assert lib.kc_graph(kc._ctx, 3, 2, None, None, ctypes.byref(st)) == KC_ERR_ARG
    assert lib.kc_graph_device(kc._ctx, 3, 2, None, 0, None, None, None) == KC_ERR_ARG
    assert lib.kc_graph(kc._ctx, 3, 3, None, None, ctypes.byref(st)) == 0
    assert st.nodes == sum(1 for t in table.values() if t == 3)
    with pytest.raises(ka.KcError) as e:
        kc.graph(5, 4)
    assert e.value.code == KC_ERR_ARG and "min_count" in str(e.value)
    # a Bloom context has no table before kc_bloom_finalize
    with ka.KmerCounter(ka.Config(k=31, bf_enable=True, est_unique=100000, min_abundance=1)) as nb:
        assert lib.kc_graph(nb._ctx, 1, 0, None, None, ctypes.byref(st)) == KC_ERR_STATE
        assert lib.kc_graph_device(nb._ctx, 1, 0, None, 0, None, None, None) == KC_ERR_STATE
        assert lib.kc_neighbors(nb._ctx, keys.ctypes.data, 4, 0, out.ctypes.data) == KC_ERR_STATE
        assert lib.kc_neighbors_device(nb._ctx, None, 0, 0, None, None) == KC_ERR_STATE
    # k = 1 has no (k - 1)-overlap
    with count(b">t\nACGTTGCA\n", 1, table_slots=1 << 12) as k1:
        assert table_of(k1) == {"A": 4, "C": 4}
        assert lib.kc_graph(k1._ctx, 1, 0, None, None, ctypes.byref(st)) == KC_ERR_ARG
        assert lib.kc_neighbors(k1._ctx, keys.ctypes.data, 4, 0, out.ctypes.data) == KC_ERR_ARG
        assert lib.kc_neighbors_device(k1._ctx, None, 0, 0, None, None) == KC_ERR_ARG
        assert lib.kc_graph_device(k1._ctx, 1, 0, None, 0, None, None, None) == KC_ERR_ARG


# ---- 6. capacity -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [31, 65])
def test_capacity_bounds_the_records(k, counted):
    import torch
    kc, table, _ = counted(k)
    flags, st = model(counted, k, 2, 0)
    W = ka.words_for_k(k)
    nodes = st["nodes"]
    cap, guard = nodes // 2, 64
    sentinel = 0x5A5A5A5A5A5A5A5A
    for capacity in (cap, nodes, 0):
        buf = torch.full(((capacity + guard) * (W + 1),), sentinel, dtype=torch.int64, device="cuda")
        n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        stats = torch.full((STAT_WORDS,), -1, dtype=torch.int64, device="cuda")
        kc.graph_device(2, 0, buf.data_ptr(), capacity, n.data_ptr(), stats.data_ptr())
        torch.cuda.synchronize()
        assert int(n.item()) == nodes
        got_st = stats.cpu().tolist()
        assert got_st == [st[f] for f in m.FIELDS] + st["side_degree"]
        host = buf.cpu().numpy().view(np.uint64)
        assert (host[capacity * (W + 1):] == np.uint64(sentinel)).all()  # nothing past the capacity
        got = records_dict(host[:capacity * (W + 1)].reshape(-1, W + 1), k)
        assert len(got) == capacity and all(got[c] == (table[c], flags[c]) for c in got)
    # statistics only: no records, no count, or neither
    stats = torch.full((STAT_WORDS,), -1, dtype=torch.int64, device="cuda")
    kc.graph_device(2, 0, 0, 0, 0, stats.data_ptr())
    n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    kc.graph_device(2, 0, 0, 1 << 40, n.data_ptr(), 0)  # (a capacity without records is not used)
    kc.graph_device(2, 0)
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == got_st and int(n.item()) == nodes


# ---- 7. neighbors ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_neighbors_every_key_width(k, counted):
    kc, table, _ = counted(k)
    rng = np.random.default_rng(k)
    held = [list(table)[i] for i in rng.choice(len(table), 1500, replace=False)]
    W = ka.words_for_k(k)
    # both strands of held k-mers, k-mers one base off (mostly absent, their neighbours mostly not)
    off = [c[:j] + "ACGT"[("ACGT".index(c[j]) + 1) % 4] + c[j + 1:] for c, j in zip(held[:500], rng.integers(0, k, 500))]
    strings = held + [m.rc(c) for c in held] + off
    got = kc.neighbors(ka.encode_kmers(strings, k))
    assert got.shape == (len(strings), 8) and got.dtype == np.uint32
    want = np.array([m.neighbors(table, x) for x in strings], dtype=np.uint32)
    assert (got == want).all()
    assert want[:1500].any(axis=1).sum() > 1400 and (want[3000:] == 0).any()
    # the other strand: R and L swap and complement
    fwd, rev = got[:1500], got[1500:3000]
    assert (rev[:, [7, 6, 5, 4, 3, 2, 1, 0]] == fwd).all()
    # for canonical keys, thresholding the counts gives the graph's edge bits
    for lo, hi in ((1, 0), (2, 50)):
        flags, _ = model(counted, k, lo, hi)
        nodes = [c for c in held if c in flags]
        cnt = got[[i for i, c in enumerate(held) if c in flags]]
        bits = ((cnt >= lo) & ((hi == 0) | (cnt <= hi))).astype(np.uint32) << np.arange(8, dtype=np.uint32)
        assert (bits.sum(axis=1) == np.array([flags[c] & 0xFF for c in nodes], dtype=np.uint32)).all()
    # a key with a bit above 2k - 1 is no k-mer
    if 2 * k % 64:
        bad = ka.encode_kmers(held[:8], k)
        bad[:, 0] |= np.uint64(1) << np.uint64(2 * k % 64)
        assert got[:8].any() and not kc.neighbors(bad).any()
    assert kc.neighbors(np.zeros((0, W), dtype=np.uint64)).shape == (0, 8)


@pytest.mark.parametrize("k", [31, 51])
def test_neighbors_of_table_keys(k):
    """the table keys route_device gives, one per window: every canonical k-mer's answer T(c) times"""
    import torch
    data = make_reads(60 + k, n_reads=500)
    img = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    chunks = ka.plan_chunks(data, k, ka.FMT_FASTA)
    W = ka.words_for_k(k)
    cap = sum((ln + 4095) // 4096 * 4096 for _, ln, _ in chunks) + len(chunks)
    cfg = dict(k=k, mode=2, min_abundance=1, table_slots=1 << 18, batch_bytes=len(data) + 4096 * (len(chunks) + 1))
    with ka.KmerCounter(ka.Config(**cfg)) as kc, ka.KmerCounter(ka.Config(**cfg)) as router:
        kc.count_device(img.data_ptr(), chunks, ka.FMT_FASTA)
        windows = kc.finish()["windows"]
        full = kc.dump()
        buf = torch.zeros(cap * W, dtype=torch.int64, device="cuda")
        n = sum(router.route_device(img.data_ptr(), chunks, ka.FMT_FASTA, 1, buf.data_ptr(), cap))
        assert n == windows
        out = torch.full((n, 8), -1, dtype=torch.int32, device="cuda")
        kc.neighbors_device(buf.data_ptr(), n, out.data_ptr(), table_keys=True)
        torch.cuda.synchronize()
        got = out.cpu().numpy().view(np.uint32)
        canon = kc.neighbors(np.ascontiguousarray(full[:, :-1]))
        want = np.repeat(canon, full[:, -1].astype(np.int64), axis=0)
        assert got.shape == want.shape and got.any()
        order = lambda a: a[np.lexsort(a.T[::-1])]
        assert (order(got) == order(want)).all()
        # a table key with word 0 == 0 is no key
        z = np.zeros((3, W), dtype=np.uint64)
        z[:, 1:] = 5
        assert not kc.neighbors(z, table_keys=True).any()


# ---- 8. ordering -----------------------------------------------------------------------------------
def test_device_forms_on_a_side_stream(counted):
    import torch
    k = 31
    kc, table, _ = counted(k)
    flags, st = model(counted, k, 1, 0)
    before = (kc.finish(), table_of(kc))
    strings = list(table)[:3000]
    keys = ka.encode_kmers(strings, k)
    want = np.array([m.neighbors(table, x) for x in strings], dtype=np.uint32)
    src = torch.from_numpy(keys.view(np.int64)).pin_memory()
    nodes = st["nodes"]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dk = torch.empty(src.shape, dtype=torch.int64, device="cuda")
        dk.copy_(src, non_blocking=True)
        out = torch.full((len(keys), 8), -1, dtype=torch.int32, device="cuda")
        kc.neighbors_device(dk.data_ptr(), len(keys), out.data_ptr(), stream=s.cuda_stream)
        recs = torch.zeros((nodes, 2), dtype=torch.int64, device="cuda")
        n = torch.full((1,), -1, dtype=torch.int64, device="cuda")
        stats = torch.full((STAT_WORDS,), -1, dtype=torch.int64, device="cuda")
        kc.graph_device(1, 0, recs.data_ptr(), nodes, n.data_ptr(), stats.data_ptr(), stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert (out.cpu().numpy().view(np.uint32) == want).all()
    assert int(n.item()) == nodes and stats.cpu().tolist() == [st[f] for f in m.FIELDS] + st["side_degree"]
    ok = same(records_dict(recs.cpu().numpy().view(np.uint64), k), {c: (table[c], f) for c, f in flags.items()})
    assert ok
    # the table is only read: no counter moved, the dump is the same
    assert kc.finish() == before[0] and table_of(kc) == before[1]
