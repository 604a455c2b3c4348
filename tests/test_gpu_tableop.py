"""GPU: table algebra (kc_table_op*, KmerCounter.table_op / table_op_device, table_compare) against
the pure-Python model tableop_model.py applied to the operands' dumps.

Inputs are generated here: two read sets drawn from two random genomes that share half their
sequence, so the two tables overlap in about half their k-mers and every count stays far below
16383 (raw count = T(c), except in the poly-A test).  Expected = the model on a.dump() / b.dump();
actual = dst.dump() as a dict and the returned statistics, compared exactly."""
import ctypes

import numpy as np
import pytest

import kaarme_amd as ka
import seq_model
import tableop_model as m

pytestmark = pytest.mark.gpu

KC_ERR_ARG, KC_ERR_TABLE_FULL, KC_ERR_STATE = -1, -3, -4
KS = [15, 31, 32, 63, 65, 479]  # W = 1 (8 slots), 1, 2, 2, 3, 15 (one slot per bucket)


# ---- inputs and helpers --------------------------------------------------------------------------
def _bases(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()


def _reads(rng, genome, n, length):
    starts = rng.integers(0, len(genome) - length + 1, n)
    return b"".join(b">r%d\n%s\n" % (i, genome[s:s + length]) for i, s in enumerate(starts))


def make_inputs(seed, n_reads=2000, read_len=100, part=20000):
    """(FASTA a, FASTA b, the shared sequence): genomes shared + own_a and shared + own_b"""
    rng = np.random.default_rng(seed)
    shared, own_a, own_b = _bases(rng, part), _bases(rng, part), _bases(rng, part)
    return (_reads(rng, shared + own_a, n_reads, read_len), _reads(rng, shared + own_b, n_reads, read_len), shared)


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


def empty(k, **cfg):
    cfg.setdefault("mode", 2)
    cfg.setdefault("table_slots", 1 << 18)
    return ka.KmerCounter(ka.Config(k=k, min_abundance=1, batch_bytes=1 << 20, **cfg))


def as_dict(kc):
    """{key words as bytes: T(c)} of dump()"""
    d = kc.dump()
    return {row[:-1].tobytes(): int(row[-1]) for row in d}


def same(got, want):
    """got == want for two big dicts, with a short account of the difference (a failed == of
    objects this size would have pytest diff their representations for minutes)"""
    if got == want:
        return True
    bad = [key for key in set(got) | set(want) if got.get(key) != want.get(key)]
    print(f"{len(got)} records against {len(want)} expected, {len(bad)} differ, e.g. "
          f"{[(key.hex(), got.get(key), want.get(key)) for key in sorted(bad)[:5]]}")
    return False


def check(dst, a_raw, b_raw, op, st, mode_a=2, mode_b=2, mode_dst=2, before=None, **ranges):
    """dst (holding `before` raw counts, default none) after one op == the model"""
    out, want = m.table_op(a_raw, b_raw, op, mode_a, mode_b, **ranges)
    assert st == want, (m.OP_NAMES[op], st, want)
    raw = m.add_into(dict(before or {}), out)
    ok = same(as_dict(dst), m.read_back(raw, mode_dst))
    assert ok, m.OP_NAMES[op]
    return raw


@pytest.fixture(scope="module")
def pairs():
    """k -> (a, b, a's dict, b's dict, a result context): three different table geometries"""
    made = {}

    def get(k):
        if k not in made:
            fa, fb, _ = make_inputs(k, 300, 600, 6000) if k > 400 else make_inputs(k)
            a, b = count(fa, k, table_slots=1 << 16), count(fb, k, table_slots=1 << 20)
            made[k] = (a, b, as_dict(a), as_dict(b), empty(k, table_slots=1 << 18))
        return made[k]

    yield get
    for a, b, _, _, dst in made.values():
        for kc in (a, b, dst):
            kc.close()


# ---- 1. every operation at every key width ----------------------------------------------------------
@pytest.mark.parametrize("op", m.OPS, ids=m.OP_NAMES)
@pytest.mark.parametrize("k", KS)
def test_every_op_every_key_width(k, op, pairs):
    a, b, da, db, dst = pairs(k)
    assert len(set(kc.finish()["table_slots"] for kc in (a, b, dst))) == 3
    assert len(set(da) & set(db)) > 1000 and len(set(da) - set(db)) > 1000 and len(set(db) - set(da)) > 1000
    dst.reset()
    st = dst.table_op(a, b, op)
    check(dst, da, db, op, st)
    assert dst.finish()["inserted"] == st["out_sum"]  # as kc_insert_counts_device counts its records


# ---- 2. a single nearly full region: keys past their home bucket -------------------------------------
@pytest.mark.parametrize("small_is", ["a", "b"])
def test_single_full_region(small_is):
    """One 4096-slot region (512 eight-slot buckets) filled to >= 0.7: tens of buckets overflow, so
    keys sit past their home bucket and the probe walks on -- and stops at the first free slot for
    the keys the table lacks.  The small table is swept (a) or probed (b; a too in a UNION)."""
    k = 31
    rng = np.random.default_rng(5)
    g1, g2 = _bases(rng, 1500), _bases(rng, 1500)
    small_fa = b">g\n" + g1 + g2 + b"\n" + _reads(rng, g1 + g2, 100, 100)
    big_fa = b">g\n" + g1 + b"\n" + _reads(rng, g1 + _bases(rng, 20000), 1500, 100)
    with count(small_fa, k, table_slots=3000) as small, count(big_fa, k, table_slots=1 << 16) as big, \
            empty(k, table_slots=1 << 20) as dst:
        st = small.finish()
        assert st["table_slots"] == 4096 and st["distinct"] >= 0.7 * 4096
        a, b = (small, big) if small_is == "a" else (big, small)
        da, db = as_dict(a), as_dict(b)
        assert len(set(da) & set(db)) > 1000
        for op in m.OPS:
            dst.reset()
            check(dst, da, db, op, dst.table_op(a, b, op))
    # the destination itself as one nearly full region
    with count(small_fa, k, table_slots=1 << 16) as a, count(big_fa, k, table_slots=1 << 16) as b, \
            empty(k, table_slots=3000) as dst:
        st = dst.table_op(a, b, m.OP_COUNTS_SUBTRACT)
        check(dst, as_dict(a), as_dict(b), m.OP_COUNTS_SUBTRACT, st)
        assert dst.finish()["table_slots"] == 4096


# ---- 3. ranges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", m.OPS, ids=m.OP_NAMES)
def test_ranges(op, pairs):
    a, b, da, db, dst = pairs(31)
    assert min(da.values()) == 1 and max(da.values()) > 3 and min(db.values()) == 1
    for ranges in (dict(a_range=(2, 0)), dict(b_range=(1, 1)), dict(b_range=(0, 1)), dict(a_range=(2, 3), b_range=(2, 0)),
                   # keys outside a's range but inside b's: a UNION yields op(0, cb) for them
                   dict(a_range=(4, 0), b_range=(1, 0))):
        dst.reset()
        check(dst, da, db, op, dst.table_op(a, b, op, **ranges), **ranges)
    if op in m.UNION_OPS:
        out, _ = m.table_op(da, db, op, a_range=(4, 0))
        low = [key for key in set(da) & set(db) if da[key] < 4]
        assert len(low) > 100 and all(out[key] == db[key] for key in low)


# ---- 4. modes -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", m.OPS, ids=m.OP_NAMES)
def test_plain_a_kaarme_b(op):
    k = 31
    fa, fb, _ = make_inputs(77)
    with count(fa, k, mode=0, table_slots=1 << 16) as a, count(fb, k, mode=2) as b, empty(k, mode=2) as dst:
        check(dst, as_dict(a), as_dict(b), op, dst.table_op(a, b, op), mode_a=0)


def test_bloom_gated_a():
    k = 31
    fa, fb, _ = make_inputs(78)
    with count(fa, k, bloom=True, est_unique=60000, fpr=0.01) as a, count(fb, k) as b, empty(k) as dst:
        da, db = as_dict(a), as_dict(b)
        plain = count(fa, k)
        assert 1000 < len(da) < len(as_dict(plain))  # the gate dropped k-mers seen once
        plain.close()
        for op in (m.OP_INTERSECT_MIN, m.OP_SUBTRACT, m.OP_UNION_SUM):
            dst.reset()
            check(dst, da, db, op, dst.table_op(a, b, op))


def test_counts_above_the_kaarme_limit():
    """Raw counts move: a poly-A k-mer counted 20000 and 17000 times reads back 16383 from either
    table, INTERSECT_SUM of the two reads back 16383 (37000 saturates in dst), COUNTS_SUBTRACT 3000."""
    k = 31
    rng = np.random.default_rng(3)
    tail = b">t\n" + _bases(rng, 500) + b"\n"
    fa = b">a\n" + b"A" * (k - 1 + 20000) + b"\n" + tail
    fb = b">b\n" + b"A" * (k - 1 + 17000) + b"\n" + tail
    poly = ka.encode_kmers(["A" * k], k)
    with count(fa, k, table_slots=1 << 16) as a, count(fb, k, table_slots=1 << 14) as b, empty(k) as dst:
        da, db = as_dict(a), as_dict(b)
        assert da[poly.tobytes()] == db[poly.tobytes()] == 16383
        ra, rb = dict(da), dict(db)
        ra[poly.tobytes()], rb[poly.tobytes()] = 20000, 17000  # the raw counts behind them
        for op, want in ((m.OP_INTERSECT_SUM, 16383), (m.OP_COUNTS_SUBTRACT, 3000), (m.OP_INTERSECT_MIN, 16383),
                         (m.OP_UNION_MAX, 16383)):
            dst.reset()
            st = dst.table_op(a, b, op)
            check(dst, ra, rb, op, st)
            assert int(dst.lookup(poly)[0]) == want
        # the ranges are on T(c): 16383 for both, whatever the raw count
        dst.reset()
        st = dst.table_op(a, b, m.OP_COUNTS_SUBTRACT, a_range=(16383, 16383), b_range=(16383, 0))
        assert st == {"a_keys": 1, "both": 1, "b_only": 0, "out_keys": 1, "out_sum": 3000}
        assert as_dict(dst) == {poly.tobytes(): 3000}


# ---- 5. state -----------------------------------------------------------------------------------------
def test_same_table_twice(pairs):
    a, _, da, _, dst = pairs(32)
    for op in m.OPS:
        dst.reset()
        check(dst, da, da, op, dst.table_op(a, a, op))


def test_emptied_operand(pairs):
    k = 31
    a, b, da, db, dst = pairs(k)
    fa, _, _ = make_inputs(k)
    with count(fa, k, table_slots=1 << 16) as gone:
        ok = same(as_dict(gone), da)
        assert ok
        gone.clear_table()
        for op in m.OPS:
            dst.reset()
            st = dst.table_op(gone, gone, op)
            assert st == dict.fromkeys(m.FIELDS, 0) and len(as_dict(dst)) == 0
            check(dst, {}, db, op, dst.table_op(gone, b, op))
            dst.reset()
            check(dst, da, {}, op, dst.table_op(a, gone, op))


def test_results_accumulate(pairs):
    a, b, da, db, dst = pairs(63)
    dst.reset()
    raw = check(dst, da, db, m.OP_INTERSECT_MIN, dst.table_op(a, b, m.OP_INTERSECT_MIN))
    raw = check(dst, da, db, m.OP_SUBTRACT, dst.table_op(a, b, m.OP_SUBTRACT), before=raw)
    assert set(raw) == set(da)
    raw = check(dst, da, db, m.OP_UNION_SUM, dst.table_op(a, b, m.OP_UNION_SUM), before=raw)
    assert dst.finish()["inserted"] == sum(raw.values())


def test_union_of_three_equals_counting_the_concatenation():
    k = 31
    f1, f2, _ = make_inputs(11, n_reads=800)
    f3, _, _ = make_inputs(12, n_reads=800)
    with count(f1, k, table_slots=1 << 16) as t1, count(f2, k, table_slots=1 << 17) as t2, count(f3, k) as t3, \
            empty(k, table_slots=1 << 20) as u12, empty(k, table_slots=1 << 19) as u123, count(f1 + f2 + f3, k) as whole:
        u12.table_op(t1, t2, m.OP_UNION_SUM)
        u123.table_op(u12, t3, m.OP_UNION_SUM)
        ok = same(as_dict(u123), as_dict(whole))
        assert ok
        assert u123.output_digest() == whole.output_digest()
        assert u123.finish()["distinct"] == whole.finish()["distinct"]
        # the same by accumulation: dst += a three times (UNION of a table with an emptied one)
        u12.reset()
        u123.clear_table()
        for t in (t1, t2, t3):
            u12.table_op(t, u123, m.OP_UNION_SUM)
        ok = same(as_dict(u12), as_dict(whole))
        assert ok


def test_statistics_without_a_destination(pairs):
    for k in (31, 65):
        a, b, da, db, _ = pairs(k)
        lib = a.lib
        for op in m.OPS:
            d, st = ka.kc_op_desc(op, 2, 0, 1, 0, 0), ka.kc_op_stats()
            assert lib.kc_table_op(None, a._ctx, b._ctx, ctypes.byref(d), ctypes.byref(st)) == 0
            assert st.as_dict() == m.table_op(da, db, op, a_range=(2, 0))[1]
        got, want = ka.table_compare(a, b), m.compare(da, db)
        assert got == want and 0 < got["jaccard"] < got["containment"] < 1
        assert ka.table_compare(a, a)["jaccard"] == 1.0
        assert ka.table_compare(a, b, a_range=(2, 0), b_range=(1, 2)) == m.compare(da, db, a_range=(2, 0), b_range=(1, 2))


def test_operands_do_not_change(pairs):
    """(dumps compared as dicts: kc_dump's record order is not fixed, its workgroups take their
    output positions from one atomic cursor)"""
    a, b, da, db, dst = pairs(31)
    before = (a.finish(), b.finish())
    for op in m.OPS:
        dst.table_op(a, b, op, a_range=(1, 5))
    ka.table_compare(a, b)
    ok_a, ok_b = same(as_dict(a), da), same(as_dict(b), db)
    assert ok_a and ok_b
    assert (a.finish(), b.finish()) == before


def test_result_is_a_counted_table():
    """compact(), seq_stats(), histogram() and lookup() work on the result as on any counted table"""
    k = 31
    fa, fb, shared = make_inputs(21)
    with count(fa, k) as a, count(fb, k) as b, empty(k, table_slots=1 << 17) as dst:
        dst.table_op(a, b, m.OP_INTERSECT_MIN)
        recs = dst.dump()
        d = {s.encode(): c for s, c in ka.decode_records(recs, k)}
        seqs = [shared[:3000], shared[10000:10400] + b"N" + shared[500:900], fa.split(b"\n")[1], b"ACGT" * 20]
        text, off = ka.pack_sequences(seqs)
        got = dst.seq_stats(seqs, solid_min=2)
        want = seq_model.seq_stats(text, off, k, d, solid_min=2)
        for i, w in enumerate(want):
            assert {n: int(got[i][n]) for n in seq_model.FIELDS} == w
        assert got[0]["present"] > 1000
        info = dst.compact()
        assert info["kmers"] == len(recs)
        crecs, _, _ = dst.compact_dump()
        ok = sorted(map(bytes, crecs)) == sorted(map(bytes, recs))
        assert ok
        assert dst.histogram().sum() == len(recs)
        # a table operation drops the snapshot: the compact representation is rebuilt from the new table
        dst.table_op(a, b, m.OP_SUBTRACT)
        with pytest.raises(ka.KcError) as e:
            dst.compact_dump()
        assert e.value.code == KC_ERR_STATE
        assert dst.compact()["kmers"] == len(as_dict(a))


# ---- 6. ordering --------------------------------------------------------------------------------------
def test_device_form_follows_the_operands_streams():
    """a is counted on a side stream and table_op_device is queued on it at once, no sync in between:
    the operation runs after the counting pass (a's own stream included) and dst's later work after it."""
    import torch
    k = 31
    fa, fb, _ = make_inputs(31, n_reads=20000)
    chunks = ka.plan_chunks(fa, k, ka.FMT_FASTA)
    batch = len(fa) + 4096 * (len(chunks) + 2)
    with ka.KmerCounter(ka.Config(k=k, min_abundance=1, table_slots=1 << 17, batch_bytes=batch)) as a, \
            count(fb, k) as b, empty(k, table_slots=1 << 20) as dst:
        db = as_dict(b)
        src = torch.frombuffer(bytearray(fa), dtype=torch.uint8).pin_memory()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            img = torch.empty(len(fa), dtype=torch.uint8, device="cuda")
            img.copy_(src, non_blocking=True)
            stats = torch.full((5,), -1, dtype=torch.int64, device="cuda")
            a.count_device(img.data_ptr(), chunks, ka.FMT_FASTA, stream=s.cuda_stream)
            dst.table_op_device(a, b, m.OP_UNION_SUM, stats_ptr=stats.data_ptr(), stream=s.cuda_stream)
        dst.sync()
        st = dict(zip(m.FIELDS, stats.cpu().tolist()))
        check(dst, as_dict(a), db, m.OP_UNION_SUM, st)
        assert st["a_keys"] > 30000


# ---- 7. errors ----------------------------------------------------------------------------------------
def test_argument_and_state_errors(pairs):
    import ctypes
    a, b, _, _, dst = pairs(31)
    other_k = pairs(32)[0]
    lib = a.lib

    def rc(d_, a_, b_, desc):
        return lib.kc_table_op(d_._ctx if d_ else None, a_._ctx if a_ else None, b_._ctx if b_ else None,
                               ctypes.byref(desc) if desc else None, None)

    ok = ka.kc_op_desc(m.OP_SUBTRACT, 1, 0, 1, 0, 0)
    dst.reset()
    assert rc(dst, a, b, ok) == 0
    assert rc(dst, a, other_k, ok) == KC_ERR_ARG and b"same k" in lib.kc_last_error(dst._ctx)
    assert rc(dst, other_k, other_k, ok) == KC_ERR_ARG
    assert rc(dst, dst, b, ok) == KC_ERR_ARG and rc(dst, a, dst, ok) == KC_ERR_ARG
    assert rc(dst, a, b, ka.kc_op_desc(7, 1, 0, 1, 0, 0)) == KC_ERR_ARG
    assert rc(dst, a, b, ka.kc_op_desc(-1, 1, 0, 1, 0, 0)) == KC_ERR_ARG
    assert rc(dst, a, b, ka.kc_op_desc(m.OP_SUBTRACT, 1, 0, 1, 0, 1)) == KC_ERR_ARG  # reserved
    assert rc(dst, a, b, ka.kc_op_desc(m.OP_SUBTRACT, 3, 2, 1, 0, 0)) == KC_ERR_ARG
    assert rc(dst, a, b, ka.kc_op_desc(m.OP_SUBTRACT, 1, 0, 9, 8, 0)) == KC_ERR_ARG
    assert rc(dst, a, b, ka.kc_op_desc(m.OP_SUBTRACT, 3, 3, 5, 0, 0)) == 0
    assert rc(dst, None, b, ok) == KC_ERR_ARG and rc(dst, a, None, ok) == KC_ERR_ARG and rc(dst, a, b, None) == KC_ERR_ARG
    # without dst the message is on a
    assert rc(None, a, other_k, ok) == KC_ERR_ARG and b"same k" in lib.kc_last_error(a._ctx)
    with pytest.raises(ka.KcError) as e:
        dst.table_op(a, b, 9)
    assert e.value.code == KC_ERR_ARG and "unknown op" in str(e.value)
    # a Bloom context has no table before kc_bloom_finalize: as a, as b and as dst
    with ka.KmerCounter(ka.Config(k=31, bf_enable=True, est_unique=100000, min_abundance=1)) as nb:
        assert rc(dst, nb, b, ok) == KC_ERR_STATE and rc(dst, a, nb, ok) == KC_ERR_STATE
        assert rc(nb, a, b, ok) == KC_ERR_STATE and rc(None, a, nb, ok) == KC_ERR_STATE
    # none of the refused calls changed dst
    assert dst.finish()["inserted"] == sum(as_dict(dst).values())


def test_destination_too_small(pairs):
    a, b, da, db, _ = pairs(31)
    with empty(31, table_slots=64) as tiny:
        assert tiny.finish()["table_slots"] == 4096 < len(set(da) | set(db))
        st = tiny.table_op(a, b, m.OP_UNION_SUM)
        assert st == m.table_op(da, db, m.OP_UNION_SUM)[1]  # the statistics are of the operation
        with pytest.raises(ka.KcError) as e:
            tiny.finish()
        assert e.value.code == KC_ERR_TABLE_FULL
