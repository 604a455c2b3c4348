"""GPU: the unitigs of the counted table (kc_unitigs*; KmerCounter.unitigs / unitig_stats /
unitigs_device) against the pure-Python model unitig_model.py applied to the table's own dump().

Expected = the model's walk on decode_records(dump()); actual = the device's records and bases.
Strand and start of a unitig are unspecified, so both sides are compared as the sorted list of
(normal, n_nodes, count_sum, circular).  Every case checks on the model that its input holds what it
claims to exercise."""
import ctypes

import numpy as np
import pytest

import graph_model as m
import kaarme_amd as ka
import unitig_model as um
from test_gpu_graph import _bases, _reads, count, make_reads, table_of

pytestmark = pytest.mark.gpu

KC_ERR_ARG, KC_ERR_STATE = -1, -4
KS = [15, 31, 32, 63, 65, 479]
RANGES = [(1, 0), (2, 0), (2, 50)]
STAT_FIELDS = ("unitigs", "circular", "nodes", "bases", "max_nodes")
HAIR = "ACGGTCAATGCCTGAAGTCCATGACCGTTAGACT"


# ---- helpers ---------------------------------------------------------------------------------------
def units_of(records, bases, k, total_bases=None):
    """[(string, n_nodes, count_sum, circular)] of device records; the offsets tile [0, bases)"""
    records = np.asarray(records, dtype=np.uint64).reshape(-1, 4)
    assert not (records[:, 3] & ~np.uint64(ka.UNITIG_CIRCULAR)).any()
    if total_bases is not None:
        order = np.argsort(records[:, 0])
        off, ln = records[order, 0].astype(np.int64), records[order, 1].astype(np.int64) + k - 1
        assert len(off) == 0 or off[0] == 0
        assert (off[1:] == off[:-1] + ln[:-1]).all() and int(ln.sum()) == total_bases
    strings = ka.unitig_strings(records, bases, k)
    return [(s, int(n), int(t), bool(f)) for s, (_, n, t, f) in zip(strings, records.tolist())]


def check_unitigs(kc, table, lo=1, hi=0, want=None):
    """kc.unitigs(lo, hi) and kc.unitig_stats(lo, hi) == the model on the table; returns the model's"""
    k = kc.cfg.k
    want = um.unitigs(table, lo, hi) if want is None else want
    records, bases, st = kc.unitigs(lo, hi)
    assert st == um.stats(want, k), (lo, hi, st, um.stats(want, k))
    assert records.shape == (st["unitigs"], 4) and bases.shape == (st["bases"],)
    got = units_of(records, bases, k, st["bases"])
    um.check_strings(got, k)
    assert um.normalised(got) == um.normalised(want), (lo, hi)
    assert kc.unitig_stats(lo, hi) == st
    gst = kc.graph_stats(lo, hi)
    assert gst["nodes"] == st["nodes"] and gst["open_unitigs"] == st["unitigs"] - st["circular"]
    return want


def claims(units, n_min=100, long_at=50):
    """more than n_min unitigs, some of long_at nodes and more, some of one node"""
    assert len(units) > n_min, len(units)
    assert any(u[1] >= long_at for u in units) and any(u[1] == 1 for u in units)


def wide_reads(seed, twice=300, once=100):
    """make_reads-style input for nine- and fifteen-word keys that forks in every range: 600-base
    reads with 1 substitution in 1000 bases from an 8 kb genome that holds a 600-base repeat
    (longer than k) three times; the first `twice` reads are emitted twice, so that their
    substitutions are still nodes from T(c) >= 2 on, the last `once` reads once, so that the range
    (1, 0) has nodes the others lack"""
    lines = make_reads(seed, twice + once, 600, 8000, rep_len=600, err=0.001).split(b"\n")
    return b"\n".join(lines[:2 * twice] * 2 + lines[2 * twice:])


@pytest.fixture(scope="module")
def counted():
    """k -> (counter, its table as a dict), made once"""
    made = {}

    def get(k):
        if k not in made:
            data = wide_reads(1000 + k) if k > 400 else make_reads(k)
            kc = count(data, k)
            made[k] = (kc, table_of(kc))
        return made[k]

    yield get
    for kc, _ in made.values():
        kc.close()


# ---- 1. every key width ----------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", RANGES)
@pytest.mark.parametrize("k", KS)
def test_every_key_width(k, lo, hi, counted):
    """(k = 479: wide_reads, since the graph test's reads for that width have no fork and no node
    at all from T(c) >= 2 on)"""
    kc, table = counted(k)
    want = um.unitigs(table, lo, hi)
    st = um.stats(want, k)
    claims(want)
    assert st["nodes"] > st["unitigs"] > 1
    check_unitigs(kc, table, lo, hi, want=want)


@pytest.mark.parametrize("k", [479, 257])
def test_wide_keys_with_forks(k):
    """fifteen- and nine-word keys on wide_reads: forks, more than 100 unitigs, long ones and
    one-node ones in every range"""
    with count(wide_reads(k), k) as kc:
        table = table_of(kc)
        for lo, hi in RANGES:
            want = um.unitigs(table, lo, hi)
            st = um.stats(want, k)
            claims(want)
            assert st["nodes"] > st["unitigs"] > 1
            assert (lo, hi) == (1, 0) or st["nodes"] < len(table)
            check_unitigs(kc, table, lo, hi, want=want)


# ---- 2. one long chain -----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [31, 127])
def test_one_long_chain(k):
    """a single 20 000-base random read is one unitig: 15 rounds of pointer jumping at k = 31"""
    rng = np.random.default_rng(2024)
    read = _bases(rng, 20000)
    with count(b">r\n" + read + b"\n", k, table_slots=1 << 16) as kc:
        table = table_of(kc)
        want = um.unitigs(table)
        assert [(u[1], u[3]) for u in want] == [(20000 - k + 1, False)]
        assert want[0][2] == 20000 - k + 1 and um.normal(*want[0][:2], False) == m.canon(read.decode())
        check_unitigs(kc, table, want=want)


# ---- 3. circles ------------------------------------------------------------------------------------
def test_circle_of_500_nodes():
    k = 31
    rng = np.random.default_rng(7)
    circle = _bases(rng, 500)
    with count(_reads(rng, circle * 3, 400, 100), k, table_slots=1 << 14) as kc:
        table = table_of(kc)
        want = um.unitigs(table)
        assert [(u[1], u[3]) for u in want] == [(500, True)]
        check_unitigs(kc, table, want=want)
        check_unitigs(kc, table, 2, 0)


def _linear():
    """reads with forks and errors"""
    return make_reads(77, n_reads=600, genome_len=8000)


def test_circles_beside_linear_reads():
    """circles of 2, 37 and 500 nodes in one table with forked linear reads and poly-A; the open
    unitigs are the same with and without the circles"""
    k = 31
    rng = np.random.default_rng(8)
    c37, c500 = _bases(rng, 37), _bases(rng, 500)
    lin = _linear()
    circles = (b">ca\n" + b"CA" * 40 + b"\n>c37\n" + c37 * 4 + b"\n" + _reads(rng, c500 * 3, 400, 100)
               + b">a\n" + b"A" * 60 + b"\n")
    with count(lin + circles, k) as kc, count(lin + b">a\n" + b"A" * 60 + b"\n", k) as plain:
        table, table0 = table_of(kc), table_of(plain)
        want, want0 = um.unitigs(table), um.unitigs(table0)
        assert sorted(u[1] for u in want if u[3]) == [2, 37, 500] and not any(u[3] for u in want0)
        claims(want0)
        assert um.stats(want0, k)["nodes"] > len(want0) > 1
        assert ("A" * k, 1, 30, False) in um.normalised(want)
        check_unitigs(kc, table, want=want)
        check_unitigs(plain, table0, want=want0)
        open_units = [u for u in um.normalised(want) if not u[3]]
        assert open_units == um.normalised(want0)
        # from the device alone, too
        got = [units_of(*c.unitigs()[:2], k) for c in (kc, plain)]
        assert [u for u in um.normalised(got[0]) if not u[3]] == um.normalised(got[1])


# ---- 4. hairpin and self edges ---------------------------------------------------------------------
def test_hairpin_and_self_edges():
    k = 31
    data = (">a\n" + "A" * 60 + "\n>ca\n" + "CA" * 40 + "\n>h\n" + HAIR + m.rc(HAIR) + "\n").encode()
    with count(data, k, table_slots=1 << 14) as kc:
        table = table_of(kc)
        want = um.unitigs(table)
        loops = [c for c in table if any(m.canon(z) == c for z in m.neighbor_strings(c))]
        assert len(loops) >= 2 and sum(1 for u in want if u[3]) == 1
        check_unitigs(kc, table, want=want)


# ---- 5. dense small k ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [2, 3, 5, 6])
def test_dense_small_k(k):
    rng = np.random.default_rng(100 + k)
    with count(b">t\n" + _bases(rng, 3000) + b"\n", k, table_slots=1 << 14) as kc:
        table = table_of(kc)
        med = int(np.median(list(table.values())))
        if k == 6:
            assert any(c == m.rc(c) for c in table)
        check_unitigs(kc, table)
        check_unitigs(kc, table, med, 0)


# ---- 6. a full table -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [31, 51])
def test_full_table(k):
    data = make_reads(40 + k)
    with count(data, k, table_slots=1 << 20) as kc0:
        distinct = kc0.finish()["distinct"]
    with count(data, k, table_slots=distinct) as kc:
        st = kc.finish()
        assert st["distinct"] == distinct and st["table_slots"] < 2 * distinct
        table = table_of(kc)
        claims(check_unitigs(kc, table, 1, 0))
        check_unitigs(kc, table, 2, 0)


# ---- 7. count semantics ----------------------------------------------------------------------------
@pytest.mark.parametrize("mode,n_a,t_a", [(0, 65536 + 2, 2), (2, 20000, 16383)])
def test_count_sum_is_of_the_reported_count(mode, n_a, t_a):
    k = 31
    rng = np.random.default_rng(11)
    tail = b"C" + _bases(rng, 400)
    data = b">a\n" + b"A" * (k - 1 + n_a) + tail + b"\n>b\n" + tail + b"\n"
    with count(data, k, mode=mode, table_slots=1 << 14) as kc:
        table = table_of(kc)
        assert table["A" * k] == t_a
        for lo, hi in ((1, 0), (t_a, t_a), (t_a + 1, 0), (2, 2)):
            want = check_unitigs(kc, table, lo, hi)
            assert (("A" * k, 1, t_a, False) in um.normalised(want)) == (lo <= t_a and (hi == 0 or t_a <= hi))


def test_bloom_gated_table():
    k = 31
    data = make_reads(5)
    with count(data, k, bloom=True, est_unique=150000, fpr=0.01) as kc:
        table = table_of(kc)
        assert len(table) > 1000
        claims(check_unitigs(kc, table), n_min=20)
        check_unitigs(kc, table, 2, 0)


# ---- 8. capacities ---------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [31, 65])
def test_capacities_bound_records_and_bases(k, counted):
    import torch
    kc, table = counted(k)
    want = um.unitigs(table, 2, 0)
    st = um.stats(want, k)
    names = set(um.normalised(want))
    n, nb, guard, sent = st["unitigs"], st["bases"], 64, 0x5A
    totals = [st[f] for f in STAT_FIELDS]
    shapes = {(u[1], u[2], u[3]) for u in want}
    for cap_u in (n // 2, n, 0):
        for cap_b in (nb // 2, nb, 0):
            recs = torch.full(((cap_u + guard) * 4,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
            bases = torch.full((cap_b + guard,), sent, dtype=torch.uint8, device="cuda")
            stats = torch.full((5,), -1, dtype=torch.int64, device="cuda")
            kc.unitigs_device(2, 0, recs.data_ptr(), cap_u, bases.data_ptr(), cap_b, stats.data_ptr())
            torch.cuda.synchronize()
            assert stats.cpu().tolist() == totals  # the totals are always full
            hr, hb = recs.cpu().numpy().view(np.uint64), bases.cpu().numpy()
            assert (hr[cap_u * 4:] == np.uint64(0x5A5A5A5A5A5A5A5A)).all() and (hb[cap_b:] == sent).all()
            written = hr[:cap_u * 4].reshape(-1, 4)
            assert len(written) == min(cap_u, n) and int(written[:, 0].max(initial=0)) < nb
            fits = (written[:, 0] + written[:, 1] + np.uint64(k - 1)) <= np.uint64(cap_b)
            got = units_of(written[fits], hb, k)
            um.check_strings(got, k)
            assert set(um.normalised(got)) <= names and len(got) == int(fits.sum())
            if cap_b == nb:
                assert fits.all()
            if cap_u == n and cap_b == nb:
                assert um.normalised(units_of(written, hb, k, nb)) == um.normalised(want)
            # every written record is a model unitig, whether its bases fit or not
            for r in written.tolist():
                assert (r[1], r[2], bool(r[3])) in shapes
            # bases of unitigs that do not fit stay untouched
            for off, nn, _, _ in written[~fits].tolist():
                lo_, hi_ = min(off, cap_b), min(off + nn + k - 1, cap_b)
                assert (hb[lo_:hi_] == sent).all()
    # statistics only
    stats = torch.full((5,), -1, dtype=torch.int64, device="cuda")
    kc.unitigs_device(2, 0, 0, 0, 0, 0, stats.data_ptr())
    kc.unitigs_device(2, 0, 0, 1 << 40, 0, 1 << 40, 0)  # (capacities without buffers are not used)
    kc.unitigs_device(2, 0)
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == totals


# ---- 9. repeatability ------------------------------------------------------------------------------
def test_two_calls_agree(counted):
    kc, _ = counted(31)
    a, b = kc.unitigs(), kc.unitigs()
    assert a[2] == b[2]
    assert um.normalised(units_of(*a[:2], 31)) == um.normalised(units_of(*b[:2], 31))


# ---- 10. ordering ----------------------------------------------------------------------------------
def test_device_form_on_a_side_stream(counted):
    import torch
    k = 31
    kc, table = counted(k)
    want = um.unitigs(table)
    st = um.stats(want, k)
    before = (kc.finish(), table_of(kc))
    src = torch.full((st["bases"],), 0x5A, dtype=torch.uint8).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        bases = torch.empty(st["bases"], dtype=torch.uint8, device="cuda")
        bases.copy_(src, non_blocking=True)  # the call's writes follow this copy on the stream
        recs = torch.zeros((st["unitigs"], 4), dtype=torch.int64, device="cuda")
        stats = torch.full((5,), -1, dtype=torch.int64, device="cuda")
        kc.unitigs_device(1, 0, recs.data_ptr(), st["unitigs"], bases.data_ptr(), st["bases"], stats.data_ptr(),
                          stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == [st[f] for f in STAT_FIELDS]
    got = units_of(recs.cpu().numpy().view(np.uint64), bases.cpu().numpy(), k, st["bases"])
    assert um.normalised(got) == um.normalised(want)
    # the table is only read: no counter moved, the dump is the same
    assert kc.finish() == before[0] and table_of(kc) == before[1]
    # the edge scratch is shared with kc_graph, which still answers
    flags, gst = m.graph(table)
    records, got_st = kc.graph()
    assert got_st == gst
    assert {c: v >> 32 for c, v in ka.decode_records(records, k)} == flags


# ---- 11. errors and states -------------------------------------------------------------------------
def test_argument_and_state_errors(counted):
    kc, table = counted(31)
    lib = kc.lib
    st = ka.kc_unitig_stats()
    assert lib.kc_unitigs(kc._ctx, 3, 2, None, None, ctypes.byref(st)) == KC_ERR_ARG
    assert lib.kc_unitigs_device(kc._ctx, 3, 2, None, 0, None, 0, None, None) == KC_ERR_ARG
    assert lib.kc_unitigs(kc._ctx, 3, 3, None, None, ctypes.byref(st)) == 0
    assert st.nodes == sum(1 for t in table.values() if t == 3)
    with pytest.raises(ka.KcError) as e:
        kc.unitigs(5, 4)
    assert e.value.code == KC_ERR_ARG and "min_count" in str(e.value)
    with ka.KmerCounter(ka.Config(k=31, bf_enable=True, est_unique=100000, min_abundance=1)) as nb:
        assert lib.kc_unitigs(nb._ctx, 1, 0, None, None, ctypes.byref(st)) == KC_ERR_STATE
        assert lib.kc_unitigs_device(nb._ctx, 1, 0, None, 0, None, 0, None, None) == KC_ERR_STATE
    with count(b">t\nACGTTGCA\n", 1, table_slots=1 << 12) as k1:
        assert lib.kc_unitigs(k1._ctx, 1, 0, None, None, ctypes.byref(st)) == KC_ERR_ARG
        assert lib.kc_unitigs_device(k1._ctx, 1, 0, None, 0, None, 0, None, None) == KC_ERR_ARG


def test_emptied_table_has_no_unitigs(counted):
    k = 31
    data = make_reads(k)
    want = um.normalised(um.unitigs(counted(k)[1]))
    zero = dict.fromkeys(STAT_FIELDS, 0)
    with count(data, k) as kc:
        assert um.normalised(units_of(*kc.unitigs()[:2], k)) == want
        for empty_it in (kc.clear_table, kc.reset):
            empty_it()
            records, bases, st = kc.unitigs()
            assert records.shape == (0, 4) and bases.shape == (0,) and st == zero
            assert kc.unitig_stats() == zero
            for off, ln, bh in ka.plan_chunks(data, k, ka.FMT_FASTA):
                kc.count_chunk(data[off:off + ln], ka.FMT_FASTA, bool(bh))
            kc.finish()
            assert um.normalised(units_of(*kc.unitigs()[:2], k)) == want
