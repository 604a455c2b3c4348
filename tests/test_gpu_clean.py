"""GPU: graph cleaning (kc_clean*; KmerCounter.clean / clean_device, clean_stats, clean_rounds) against
the pure-Python model clean_model.py applied to the source table's own dump().

Expected = the model on decode_records(src.dump()), on raw counts; actual = the destination's dump as
a dict (every destination is created with -a 1) and the returned statistics, compared exactly.  Every
case first checks on the model that its input holds what it claims to exercise."""
import ctypes

import numpy as np
import pytest

import cdbg_model as cm
import clean_cases as cc
import clean_model as clm
import graph_model as m
import kaarme_amd as ka
from test_gpu_cdbg import check_cdbg
from test_gpu_graph import _bases, _reads, count, make_reads, same, table_of
from test_gpu_unitig import HAIR, wide_reads

pytestmark = pytest.mark.gpu

KC_ERR_ARG, KC_ERR_TABLE_FULL, KC_ERR_STATE = -1, -3, -4
KS = [15, 31, 32, 63, 65, 479]
RANGES = [(1, 0), (2, 0), (2, 50)]
ZERO = dict.fromkeys(clm.FIELDS, 0)


# ---- helpers ---------------------------------------------------------------------------------------
def fresh(k, slots=1 << 18, mode=2):
    """an empty destination that outputs every k-mer it holds"""
    return ka.KmerCounter(ka.Config(k=k, mode=mode, min_abundance=1, table_slots=slots, batch_bytes=1 << 20))


def add_into(total, kept):
    for c, v in kept.items():
        total[c] = total.get(c, 0) + v
    return total


def check_clean(dst, src, table, lo=1, hi=0, graph=None, raw=None, before=None, **rule):
    """dst (holding `before`, default nothing) after dst.clean(src, lo, hi, **rule) == the model on the
    table; returns (the model's kept table, the statistics)"""
    want, want_st = clm.clean(table, lo, hi, raw=raw, graph=graph, **rule)
    st = dst.clean(src, lo, hi, **rule)
    assert st == want_st, (lo, hi, rule, st, want_st)
    ok = same(table_of(dst), add_into(dict(before or {}), want))
    assert ok, (lo, hi, rule)
    return want, st


def shape(table, lo=1, hi=0, graph=None):
    """sorted [(n_nodes, category or "-")] of the range's unitigs"""
    units, edges, _ = graph or cm.cdbg(table, lo, hi)
    return sorted((u[1], clm.category(u, d) or "-") for u, d in zip(units, clm.end_degrees(units, edges)))


@pytest.fixture(scope="module")
def counted():
    """k -> (counter, its table as a dict), made once; .model(k, lo, hi) -> the model's graph, made once.
    The inputs are test_gpu_cdbg's: at every k of KS they have short tips in every range and short
    isolated unitigs from T(c) >= 2 on (test_every_key_width asserts it), so none is added by hand."""
    made, models = {}, {}

    def get(k):
        if k not in made:
            data = wide_reads(1000 + k) if k > 400 else make_reads(k)
            kc = count(data, k)
            made[k] = (kc, table_of(kc))
        return made[k]

    def model(k, lo=1, hi=0):
        if (k, lo, hi) not in models:
            models[k, lo, hi] = cm.cdbg(get(k)[1], lo, hi)
        return models[k, lo, hi]

    get.model = model
    yield get
    for kc, _ in made.values():
        kc.close()


# ---- 1. every key width ----------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", RANGES)
@pytest.mark.parametrize("k", KS)
def test_every_key_width(k, lo, hi, counted):
    kc, table = counted(k)
    graph = counted.model(k, lo, hi)
    rule = dict(tip_max_nodes=k - 1, iso_max_nodes=k - 1)
    want, want_st = clm.clean(table, lo, hi, graph=graph, **rule)
    assert want_st["tips"] > 0 and 0 < want_st["out_keys"] < want_st["nodes"]
    if (lo, hi) == (2, 0):
        assert want_st["isolated"] > 0
    with fresh(k, 1 << 17) as dst:
        assert dst.finish()["table_slots"] != kc.finish()["table_slots"]  # the keys move between two geometries
        check_clean(dst, kc, table, lo, hi, graph=graph, **rule)
        ust = kc.unitig_stats(lo, hi)
        assert (want_st["unitigs"], want_st["nodes"]) == (ust["unitigs"], ust["nodes"])
        assert ka.clean_stats(kc, lo, hi, **rule) == want_st
        assert dst.finish()["inserted"] == want_st["out_sum"]


@pytest.mark.parametrize("W", [W for W in range(1, 16) if W not in {ka.words_for_k(k) for k in KS}])
def test_the_other_key_widths(W):
    """the widest key of every width that KS does not reach (k = 32 W - 1, W = 4 .. 14), on the width
    tests' input, from T(c) >= 2 on"""
    import key_widths as kw
    k = kw.K_HI[W]
    with count(kw.width_input(k), k) as src, fresh(k, 1 << 17) as dst:
        table = table_of(src)
        _, st = check_clean(dst, src, table, 2, 0, tip_max_nodes=k - 1, iso_max_nodes=k - 1)
        assert st["tips"] + st["isolated"] > 0 and st["out_keys"] > 0


# ---- 2. hand-built graphs --------------------------------------------------------------------------
def test_cascade_over_three_rounds():
    k, n = 31, 30
    seqs, b, c = cc.cascade(k, n=n)
    with count(cc.fasta(seqs), k, table_slots=1 << 14) as src:
        table = table_of(src)
        assert shape(table) == [(n, "-"), (n, "tip"), (n, "tip"), (40, "tip"), (50, "tip")]
        want, want_st = clm.model_rounds(table, 5, tip_max_nodes=n)
        assert [(s["tips"], s["tip_nodes"]) for s in want_st] == [(2, 2 * n), (1, n), (0, 0)]
        assert shape(want) == [(90, "isolated")]
        out, st = ka.clean_rounds(src, 5, tip_max_nodes=n)
        with out:
            assert st == want_st and table_of(out) == want
            assert out.finish()["table_slots"] >= len(want)
        # one round only: the near piece is still there
        want1, want_st1 = clm.model_rounds(table, 1, tip_max_nodes=n)
        out, st = ka.clean_rounds(src, 1, tip_max_nodes=n)
        with out:
            assert st == want_st1 == want_st[:1] and table_of(out) == want1 and len(want1) == 90 + n
        assert table_of(src) == table  # the source is not closed and not changed


def test_bubble_keeps_both_arms():
    k = 31
    seqs, _ = cc.bubble(k)
    with count(cc.fasta(seqs), k, table_slots=1 << 14) as src, fresh(k, 1 << 14) as dst:
        table = table_of(src)
        assert shape(table) == [(100 - 50 - k, "tip"), (k, "-"), (k, "-"), (50, "tip")]
        want, st = check_clean(dst, src, table, tip_max_nodes=k - 1, iso_max_nodes=k - 1)
        # (the 19 nodes behind the bubble are a short tip; both arms stay)
        assert (st["tips"], st["tip_nodes"], st["isolated"]) == (1, 100 - 50 - k, 0) and len(want) == 50 + 2 * k
        dst.reset()
        want, st = check_clean(dst, src, table, tip_max_nodes=10, iso_max_nodes=k - 1)
        assert want == table and st["tips"] == 0


def test_junction_of_two_short_tips_loses_both():
    k = 31
    seqs, stem = cc.two_tip_junction(k)
    with count(cc.fasta(seqs), k, table_slots=1 << 14) as src, fresh(k, 1 << 14) as dst:
        table = table_of(src)
        assert shape(table) == [(3, "tip"), (3, "tip"), (50, "tip")]
        want, st = check_clean(dst, src, table, tip_max_nodes=k - 1)
        assert (st["tips"], st["tip_nodes"]) == (2, 6) and len(want) == 50 and set(want.values()) == {2}


def test_circle_of_500_nodes_is_kept():
    k = 31
    rng = np.random.default_rng(7)
    circle = _bases(rng, 500)
    with count(_reads(rng, circle * 3, 400, 100), k, table_slots=1 << 14) as src, fresh(k, 1 << 14) as dst:
        table = table_of(src)
        units, _, _ = cm.cdbg(table)
        assert [(u[1], u[3]) for u in units] == [(500, True)]
        want, st = check_clean(dst, src, table, tip_max_nodes=1000, iso_max_nodes=1000)
        assert want == table and (st["unitigs"], st["tips"], st["isolated"], st["out_keys"]) == (1, 0, 0, 500)


def test_one_long_chain_above_and_below_the_limit():
    k = 31
    rng = np.random.default_rng(2024)
    n = 20000 - k + 1
    with count(b">r\n" + _bases(rng, 20000) + b"\n", k, table_slots=1 << 16) as src, fresh(k, 1 << 16) as dst:
        table = table_of(src)
        graph = cm.cdbg(table)
        assert shape(table, graph=graph) == [(n, "isolated")]
        want, st = check_clean(dst, src, table, graph=graph, iso_max_nodes=n - 1, tip_max_nodes=n)
        assert want == table and st["isolated"] == 0
        dst.reset()
        want, st = check_clean(dst, src, table, graph=graph, iso_max_nodes=n)
        assert want == {} and (st["isolated"], st["isolated_nodes"], st["out_keys"], st["out_sum"]) == (1, n, 0, 0)


def test_hairpin_and_self_edges_count_as_connected():
    k = 31
    data = (">a\n" + "A" * 60 + "\n>ca\n" + "CA" * 40 + "\n>h\n" + HAIR + m.rc(HAIR) + "\n").encode()
    with count(data, k, table_slots=1 << 14) as src, fresh(k, 1 << 14) as dst:
        table = table_of(src)
        units, edges, _ = cm.cdbg(table)
        own = {e[0] for e in edges if e[0] == e[2]}
        cats = {u[1]: clm.category(u, d) for u, d in zip(units, clm.end_degrees(units, edges))}
        # poly-A (one node, a loop on either side), the hairpin (a dead end and an edge into itself), the CA circle
        assert len(own) == 2 and cats[1] is None and "isolated" not in cats.values() and "tip" in cats.values()
        assert any(u[3] for u in units)
        want, st = check_clean(dst, src, table, iso_max_nodes=1000)
        assert want == table and st["isolated"] == 0
        dst.reset()
        want, st = check_clean(dst, src, table, tip_max_nodes=k - 1, iso_max_nodes=k - 1)
        assert st["tips"] == 1 and st["tip_nodes"] == max(n for n, c in cats.items() if c == "tip") <= k - 1


# ---- 3. dense small k ------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n", [(4, 300), (6, 3000)])
def test_dense_small_k(k, n):
    """palindromic nodes with neighbours, self loops and sides of degree 4"""
    rng = np.random.default_rng(200 + k)
    with count(b">t\n" + _bases(rng, n) + b"\n", k, table_slots=1 << 14) as src, fresh(k, 1 << 14) as dst:
        table = table_of(src)
        med = int(np.median(list(table.values())))
        nodes = set(table)
        assert any(m.edge_info(nodes, c)[0] for c in nodes if c == m.rc(c))
        removed = 0
        for lo, hi in ((1, 0), (med, 0), (1, med)):
            graph = cm.cdbg(table, lo, hi)
            for rule in (dict(tip_max_nodes=3, iso_max_nodes=3), dict(tip_max_nodes=100, iso_max_nodes=100, max_mean=med)):
                dst.reset()
                _, st = check_clean(dst, src, table, lo, hi, graph=graph, **rule)
                removed += st["tips"] + st["isolated"]
        assert removed > 0


# ---- 4. the guard ----------------------------------------------------------------------------------
def test_guard_keeps_the_heavy_tip():
    k, t = 31, 5
    rng = np.random.default_rng(12)
    g = cc.rand(rng, 120 + k - 1)
    light, heavy = cc.branch(rng, g, 40, t, k), cc.branch(rng, g, 80, t, k)
    with count(cc.fasta([g, light] + [heavy] * 10), k, table_slots=1 << 14) as src, fresh(k, 1 << 14) as dst:
        table = table_of(src)
        assert shape(table) == [(t, "tip"), (t, "tip"), (40, "-"), (40, "tip"), (40, "tip")]
        n_light = {m.canon(light[i:i + k]) for i in range(t)}
        n_heavy = {m.canon(heavy[i:i + k]) for i in range(t)}
        assert all(table[c] == 1 for c in n_light) and all(table[c] == 10 for c in n_heavy)
        want, st = check_clean(dst, src, table, tip_max_nodes=t, max_mean=5)
        assert set(table) - set(want) == n_light and (st["tips"], st["tip_nodes"]) == (1, t)
        dst.reset()
        want, st = check_clean(dst, src, table, tip_max_nodes=t)
        assert set(table) - set(want) == n_light | n_heavy and (st["tips"], st["tip_nodes"]) == (2, 2 * t)
        dst.reset()
        want, st = check_clean(dst, src, table, tip_max_nodes=t, max_mean=10)  # 50 <= 10 * 5
        assert st["tips"] == 2


# ---- 5. what is added, and to what -----------------------------------------------------------------
def test_both_rules_off_copies_the_range(counted):
    k = 31
    kc, table = counted(k)
    with fresh(k) as dst:
        for lo, hi in ((2, 0), (2, 50)):
            dst.reset()
            want, st = check_clean(dst, kc, table, lo, hi, graph=counted.model(k, lo, hi))
            assert want == {c: t for c, t in table.items() if m.in_range(t, lo, hi)} and 0 < len(want) < len(table)
            assert (st["tips"], st["isolated"], st["out_keys"]) == (0, 0, st["nodes"])


def test_results_accumulate_and_drop_the_compact_snapshot(counted):
    k = 31
    kc, table = counted(k)
    graph = counted.model(k, 2, 0)
    rule = dict(tip_max_nodes=k - 1, iso_max_nodes=k - 1)
    with fresh(k) as dst:
        want, st = check_clean(dst, kc, table, 2, 0, graph=graph, **rule)
        assert dst.compact()["kmers"] == len(want)
        total = add_into({}, want)
        want2, st2 = check_clean(dst, kc, table, 2, 0, graph=graph, before=total)  # the rules off: more keys
        total = add_into(total, want2)
        assert len(want2) > len(want) and set(total) == set(want2)
        assert dst.finish()["inserted"] == st["out_sum"] + st2["out_sum"] == sum(total.values())
        with pytest.raises(ka.KcError) as e:  # the snapshot was of the table before the calls
            dst.compact_dump()
        assert e.value.code == KC_ERR_STATE
        assert dst.compact()["kmers"] == len(total)


def test_no_destination_and_source_untouched(counted):
    k = 31
    kc, table = counted(k)
    rule = dict(tip_max_nodes=k - 1, iso_max_nodes=k - 1, max_mean=40)
    before = (kc.output_digest(), kc.finish())
    want, want_st = clm.clean(table, 2, 0, graph=counted.model(k, 2, 0), **rule)
    assert ka.clean_stats(kc, 2, 0, **rule) == want_st
    d, st = ka.kc_clean_desc(2, 0, k - 1, k - 1, 40, 0), ka.kc_clean_stats()
    assert kc.lib.kc_clean(None, kc._ctx, ctypes.byref(d), ctypes.byref(st)) == 0 and st.as_dict() == want_st
    assert kc.lib.kc_clean(None, kc._ctx, ctypes.byref(d), None) == 0
    assert kc.lib.kc_clean_device(None, kc._ctx, ctypes.byref(d), None, None) == 0
    assert (kc.output_digest(), kc.finish()) == before
    with fresh(k) as dst:
        was = dst.finish()["inserted"]
        st = dst.clean(kc, 2, 0, **rule)
        assert st == want_st and dst.finish()["inserted"] == was + st["out_sum"]
        assert (kc.output_digest(), kc.finish()) == before
        ok = same(table_of(kc), table)
        assert ok


def test_counts_above_the_kaarme_limit():
    """Raw counts move: a poly-A k-mer counted 20000 times reads back 16383 from the -m 2 source and
    20000 mod 65536 from a -m 0 destination."""
    k = 31
    rng = np.random.default_rng(11)
    tail = b"C" + _bases(rng, 400)
    data = b">a\n" + b"A" * (k - 1 + 20000) + tail + b"\n>b\n" + tail + b"\n"
    with count(data, k, mode=2, table_slots=1 << 14) as src, fresh(k, 1 << 14, mode=0) as dst:
        table = table_of(src)
        assert table["A" * k] == 16383
        raw = {"A" * k: 20000}
        want, st = check_clean(dst, src, table, raw=raw, tip_max_nodes=k - 1, iso_max_nodes=k - 1)
        assert want["A" * k] == 20000 == 20000 % 65536 and st["out_sum"] == sum(want.values())
        assert int(dst.lookup(ka.encode_kmers(["A" * k], k))[0]) == 20000
        # the range and the guard are on T(c): 16383
        dst.reset()
        want, st = check_clean(dst, src, table, 16383, 16383, raw=raw)
        assert want == {"A" * k: 20000} and st["out_sum"] == 20000


# ---- 6. more table states --------------------------------------------------------------------------
def test_bloom_gated_source():
    k = 31
    with count(make_reads(5), k, bloom=True, est_unique=150000, fpr=0.01) as src, fresh(k) as dst:
        table = table_of(src)
        assert len(table) > 1000
        _, st = check_clean(dst, src, table, tip_max_nodes=k - 1, iso_max_nodes=k - 1)
        assert st["tips"] + st["isolated"] > 0


def test_emptied_source_adds_nothing():
    k = 31
    data = make_reads(k)
    with count(data, k) as src, fresh(k) as dst:
        assert ka.clean_stats(src, tip_max_nodes=k - 1)["nodes"] > 1000
        for empty_it in (src.clear_table, src.reset):
            empty_it()
            assert dst.clean(src, tip_max_nodes=k - 1, iso_max_nodes=k - 1) == ZERO
            assert ka.clean_stats(src) == ZERO and table_of(dst) == {} and dst.finish()["inserted"] == 0
            for off, ln, bh in ka.plan_chunks(data, k, ka.FMT_FASTA):
                src.count_chunk(data[off:off + ln], ka.FMT_FASTA, bool(bh))
            src.finish()


def test_full_source_table():
    k = 31
    data = make_reads(40 + k)
    with count(data, k, table_slots=1 << 20) as kc0:
        distinct = kc0.finish()["distinct"]
    with count(data, k, table_slots=distinct) as src, fresh(k) as dst:
        fin = src.finish()
        assert fin["distinct"] == distinct and fin["table_slots"] < 2 * distinct
        table = table_of(src)
        _, st = check_clean(dst, src, table, 2, 0, tip_max_nodes=k - 1, iso_max_nodes=k - 1)
        assert st["tips"] > 0


# ---- 7. the result is a counted table --------------------------------------------------------------
def test_result_is_a_counted_table(counted):
    k = 31
    kc, table = counted(k)
    rule = dict(tip_max_nodes=k - 1, iso_max_nodes=k - 1)
    want, want_st = clm.clean(table, 2, 0, graph=counted.model(k, 2, 0), **rule)
    out, st = ka.clean_rounds(kc, 1, min_count=2, **rule)
    with out:
        assert st == [want_st] and out.cfg.table_slots == len(want) + len(want) // 8 + 4096
        units, edges, cst = check_cdbg(out, want)
        assert cst["nodes"] == len(want) and cst["unitigs"] < want_st["unitigs"]  # tips gone, their junctions closed
        assert int(out.histogram().sum()) == len(want)
        # a further round works on it as on any counted table
        again, st2 = check_clean_fresh(out, want, **rule)
        assert st2["nodes"] == len(want)


def check_clean_fresh(src, table, **rule):
    with fresh(src.cfg.k) as dst:
        return check_clean(dst, src, table, **rule)


# ---- 8. ordering -----------------------------------------------------------------------------------
def test_device_form_on_a_side_stream(counted):
    import torch
    k = 31
    kc, table = counted(k)
    rule = dict(tip_max_nodes=k - 1, iso_max_nodes=k - 1)
    want, want_st = clm.clean(table, 2, 0, graph=counted.model(k, 2, 0), **rule)
    before = (kc.finish(), kc.output_digest())
    with fresh(k) as dst:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            stats = torch.full((8,), -1, dtype=torch.int64, device="cuda")
            dst.clean_device(kc, 2, 0, stats_ptr=stats.data_ptr(), stream=s.cuda_stream, **rule)
            dst.clean_device(kc, 2, 0, stream=s.cuda_stream, **rule)  # (without statistics)
        dst.sync()
        torch.cuda.synchronize()
        assert dict(zip(clm.FIELDS, stats.cpu().tolist())) == want_st
        ok = same(table_of(dst), add_into(dict(want), want))
        assert ok
        assert dst.finish()["inserted"] == 2 * want_st["out_sum"]
    assert (kc.finish(), kc.output_digest()) == before


# ---- 9. errors ---------------------------------------------------------------------------------------
def test_argument_and_state_errors(counted):
    kc, table = counted(31)
    other_k = counted(32)[0]
    lib = kc.lib

    def rcs(d_, s_, desc):
        """the codes of the host form and of the device form"""
        p = [d_._ctx if d_ else None, s_._ctx if s_ else None, ctypes.byref(desc) if desc else None]
        return lib.kc_clean(*p, None), lib.kc_clean_device(*p, None, None)

    ok = ka.kc_clean_desc(2, 0, 30, 30, 0, 0)
    with fresh(31) as dst:
        assert rcs(dst, kc, ok) == (0, 0)
        filled = table_of(dst)
        arg, state = (KC_ERR_ARG,) * 2, (KC_ERR_STATE,) * 2
        assert rcs(dst, dst, ok) == arg and rcs(kc, kc, ok) == arg
        assert rcs(dst, other_k, ok) == arg and b"same k" in lib.kc_last_error(dst._ctx)
        assert rcs(dst, kc, ka.kc_clean_desc(2, 0, 30, 30, 0, 1)) == arg and b"reserved" in lib.kc_last_error(dst._ctx)
        assert rcs(dst, kc, ka.kc_clean_desc(3, 2, 30, 30, 0, 0)) == arg and b"min_count" in lib.kc_last_error(dst._ctx)
        assert rcs(dst, kc, ka.kc_clean_desc(3, 3, 30, 30, 0, 0)) == (0, 0)
        filled = add_into(add_into(filled, clm.clean(table, 3, 3, tip_max_nodes=30, iso_max_nodes=30)[0]),
                          clm.clean(table, 3, 3, tip_max_nodes=30, iso_max_nodes=30)[0])
        assert rcs(dst, None, ok) == arg and rcs(dst, kc, None) == arg and rcs(None, None, ok) == arg
        # without dst the message is on src
        assert rcs(None, kc, ka.kc_clean_desc(3, 2, 0, 0, 0, 0)) == arg and b"min_count" in lib.kc_last_error(kc._ctx)
        with pytest.raises(ka.KcError) as e:
            dst.clean(kc, 5, 4)
        assert e.value.code == KC_ERR_ARG and "min_count" in str(e.value)
        # k < 2
        with count(b">t\nACGTTGCA\n", 1, table_slots=1 << 12) as k1, fresh(1, 1 << 12) as d1:
            assert rcs(d1, k1, ka.kc_clean_desc(1, 0, 0, 0, 0, 0)) == arg and rcs(None, k1, ok) == arg
        # a Bloom context has no table before kc_bloom_finalize: as src and as dst
        with ka.KmerCounter(ka.Config(k=31, bf_enable=True, est_unique=100000, min_abundance=1)) as nb:
            assert rcs(dst, nb, ok) == state and rcs(None, nb, ok) == state and rcs(nb, kc, ok) == state
        # none of the refused calls changed dst
        ok_ = same(table_of(dst), filled)
        assert ok_
        assert dst.finish()["inserted"] == sum(filled.values())


def test_destination_too_small(counted):
    k = 31
    kc, table = counted(k)
    want, want_st = clm.clean(table, 1, 0, graph=counted.model(k, 1, 0), tip_max_nodes=3)
    with fresh(k, slots=64) as tiny:
        assert tiny.finish()["table_slots"] == 4096 < want_st["out_keys"]
        assert tiny.clean(kc, tip_max_nodes=3) == want_st  # the statistics are of the cleaning
        with pytest.raises(ka.KcError) as e:
            tiny.finish()
        assert e.value.code == KC_ERR_TABLE_FULL
