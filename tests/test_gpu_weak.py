"""GPU: weak-link removal (kc_cut_weak*; KmerCounter.cut_weak / cut_weak_device, weak_stats,
weak_rounds) against the pure-Python model weak_model.py applied to the source table's own dump().

Expected = the model on decode_records(src.dump()), on raw counts; actual = the destination's dump as
a dict (every destination is created with -a 1) and the returned statistics, compared exactly.  Every
case first checks on the model that its input holds what it claims to exercise."""
import ctypes

import numpy as np
import pytest

import bubble_cases as bc
import bubble_model as bm
import cdbg_model as cm
import clean_cases as cc
import clean_model as clm
import kaarme_amd as ka
import weak_cases as wc
import weak_model as wm
from test_gpu_cdbg import check_cdbg
from test_gpu_clean import add_into, fresh
from test_gpu_graph import _bases, _reads, count, make_reads, same, table_of
from test_weak_model import double_neighbour_claims, nodes_of, palindrome_claims, unit_of

pytestmark = pytest.mark.gpu

KC_ERR_ARG, KC_ERR_TABLE_FULL, KC_ERR_STATE = -1, -3, -4
KS = [15, 31, 32, 63, 65, 479]
READ_KS = [15, 31, 32]
ZERO = dict.fromkeys(wm.FIELDS, 0)


# ---- helpers ---------------------------------------------------------------------------------------
def check_cut(dst, src, table, lo=1, hi=0, graph=None, raw=None, before=None, **rule):
    """dst (holding `before`, default nothing) after dst.cut_weak(src, lo, hi, **rule) == the model on
    the table; returns (the model's kept table, the statistics)"""
    want, want_st = wm.cut(table, lo, hi, raw=raw, graph=graph, **rule)
    st = dst.cut_weak(src, lo, hi, **rule)
    assert st == want_st, (lo, hi, rule, st, want_st)
    ok = same(table_of(dst), add_into(dict(before or {}), want))
    assert ok, (lo, hi, rule)
    return want, st


def counted_cases(seqs, k, slots=1 << 14, **cfg):
    return count(cc.fasta(seqs), k, table_slots=slots, **cfg)


@pytest.fixture(scope="module")
def counted():
    """k -> (counter of make_reads(k), its table as a dict), made once; .model(k, lo, hi) -> the model's
    graph, made once"""
    made, models = {}, {}

    def get(k):
        if k not in made:
            kc = count(make_reads(k), k)
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
def _widths():
    import key_widths as kw
    return KS + [kw.K_HI[W] for W in range(1, 16) if W not in {ka.words_for_k(k) for k in KS}]


def test_the_widths_are_all_fifteen():
    assert {ka.words_for_k(k) for k in _widths()} == set(range(1, 16))


@pytest.mark.parametrize("k", _widths())
def test_every_key_width(k):
    seqs, j = wc.chimera(k)
    with counted_cases(seqs, k, 1 << 15) as src, fresh(k, 1 << 17) as dst:
        assert dst.finish()["table_slots"] != src.finish()["table_slots"]  # the keys move between two geometries
        table = table_of(src)
        for lo, hi in ((1, 0), (2, 0)):
            graph = cm.cdbg(table, lo, hi)
            rule = dict(max_nodes=k, ratio_permille=200)
            want, want_st = wm.cut(table, lo, hi, graph=graph, **rule)
            if lo == 1:
                assert (want_st["unitigs"], want_st["interior"], want_st["weak"], want_st["cut"]) == (5, 1, 1, 1)
                assert set(table) - set(want) == nodes_of(j, k) and want_st["cut_nodes"] == k - 1
            else:  # the joint is given once: from T(c) >= 2 on the graph is G1 and G2
                assert (want_st["unitigs"], want_st["interior"], want_st["cut"]) == (2, 0, 0)
            dst.reset()
            check_cut(dst, src, table, lo, hi, graph=graph, **rule)
            assert ka.weak_stats(src, lo, hi, **rule) == want_st
            assert dst.finish()["inserted"] == want_st["out_sum"]
        # what is left is G1 and G2
        units, _, cst = check_cdbg(dst, want)
        assert sorted((u[1], u[3]) for u in units) == [(100, False), (100, False)]


# ---- 2. real read errors ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", READ_KS)
def test_read_errors(k, counted):
    kc, table = counted(k)
    graph = counted.model(k)
    with fresh(k) as dst:
        want, st = check_cut(dst, kc, table, graph=graph, max_nodes=k, ratio_permille=200)
        assert st["interior"] > st["weak"] >= st["cut"] > 0
        dst.reset()
        _, st1 = check_cut(dst, kc, table, graph=graph, max_nodes=2 * k, ratio_permille=1000)
        assert st1["cut"] > st["cut"]


# ---- 3. the cases of weak_cases --------------------------------------------------------------------
def test_threshold_is_strict():
    k = 31
    seqs, j = wc.chimera(k, light=2)
    with counted_cases(seqs, k) as src, fresh(k, 1 << 14) as dst:
        table = table_of(src)
        graph = cm.cdbg(table)
        units, edges, _ = graph
        u = unit_of(units, j, k)
        s, n = wm.local(units, wm.neighbours(units, edges)[u])
        assert units[u][2] * n * 1000 == 200 * s * units[u][1]  # the two sides are equal
        want, st = check_cut(dst, src, table, graph=graph, max_nodes=k, ratio_permille=200)
        assert want == table and (st["interior"], st["weak"], st["cut"]) == (1, 0, 0)
        dst.reset()
        want, st = check_cut(dst, src, table, graph=graph, max_nodes=k, ratio_permille=201)
        assert set(table) - set(want) == nodes_of(j, k) and (st["weak"], st["cut"]) == (1, 1)


def test_het_bubble_loses_both_arms_at_a_high_ratio():
    k = 31
    seqs, q = wc.het_bubble(k)
    with counted_cases(seqs, k) as src, fresh(k, 1 << 14) as dst:
        table = table_of(src)
        graph = cm.cdbg(table)
        assert len(graph[0]) == 4 and len(wm.interior(*graph[:2])) == 2
        want, st = check_cut(dst, src, table, graph=graph, max_nodes=k, ratio_permille=200)
        assert want == table and (st["interior"], st["weak"], st["cut"]) == (2, 0, 0)
        dst.reset()
        want, st = check_cut(dst, src, table, graph=graph, max_nodes=k, ratio_permille=600)
        assert (st["weak"], st["cut"], st["cut_nodes"]) == (2, 2, 2 * k)


def test_a_neighbour_reached_twice_counts_twice():
    k = 31
    seqs, b, v, w = wc.double_neighbour(k)
    with counted_cases(seqs, k) as src, fresh(k, 1 << 14) as dst:
        table = table_of(src)
        graph = cm.cdbg(table)
        double_neighbour_claims(table, graph, b, v, w, k)
        want, st = check_cut(dst, src, table, graph=graph, max_nodes=2 * k, ratio_permille=300)
        assert set(table) - set(want) == nodes_of(b, k) and st["cut"] == 1


def test_edges_back_into_the_unitig_give_no_entry():
    k = 31
    with counted_cases(wc.SELF_LOOPS, k) as src, fresh(k, 1 << 14) as dst:
        table = table_of(src)
        graph = cm.cdbg(table)
        units, edges, _ = graph
        a = unit_of(units, "A" * k, k)
        assert wm.interior(units, edges) == {a} and wm.neighbours(units, edges)[a] == []
        assert any(u[3] for u in units) and "tip" in {clm.category(u, d) for u, d in zip(units, clm.end_degrees(units, edges))}
        want, st = check_cut(dst, src, table, graph=graph, max_nodes=1000, max_mean=1000)
        assert want == table and (st["interior"], st["weak"], st["cut"]) == (1, 0, 0)
    seqs, t = wc.loop_end(k)
    with counted_cases(seqs, k) as src, fresh(k, 1 << 14) as dst:
        table = table_of(src)
        graph = cm.cdbg(table)
        units, edges, _ = graph
        a = unit_of(units, "A" * k, k)
        assert sum(clm.end_degrees(units, edges)[a]) == 3 and len(wm.neighbours(units, edges)[a]) == 1
        want, st = check_cut(dst, src, table, graph=graph, max_nodes=1, ratio_permille=500)
        assert want == table and (st["interior"], st["weak"]) == (1, 0)
        dst.reset()
        want, st = check_cut(dst, src, table, graph=graph, max_nodes=1, ratio_permille=501)
        assert set(table) - set(want) == {"A" * k} and st["cut"] == 1


def test_palindromic_unitig_is_kept_and_counts_as_a_neighbour():
    k = 32
    seqs, p, x_unit = wc.palindrome(k)
    with counted_cases(seqs, k) as src, fresh(k, 1 << 14) as dst:
        table = table_of(src)
        graph = cm.cdbg(table)
        palindrome_claims(table, graph, p, x_unit, k)
        want, st = check_cut(dst, src, table, graph=graph, max_nodes=1000, ratio_permille=1000)
        assert p in want and nodes_of(x_unit, k) <= set(want)


@pytest.mark.parametrize("k,length,sites,seeds", [(6, 100, 8, (130, 160, 0, 1, 2, 3)), (8, 400, 20, (21, 0, 1))])
def test_dense_small_k(k, length, sites, seeds):
    """accidental repeats, self loops and palindromic nodes"""
    cut = 0
    with fresh(k, 1 << 14) as dst:
        for seed in seeds:
            with counted_cases(bc.dense(k, seed, length, sites), k) as src:
                table = table_of(src)
                for lo in (1, 2):
                    graph = cm.cdbg(table, lo, 0)
                    for rule in (dict(max_nodes=k, ratio_permille=200), dict(max_nodes=2 * k, ratio_permille=1000),
                                 dict(max_nodes=3 * k, max_mean=1), dict(max_nodes=3 * k, ratio_permille=600, max_mean=2)):
                        dst.reset()
                        cut += check_cut(dst, src, table, lo, 0, graph=graph, **rule)[1]["cut"]
    assert cut > 0


def test_big_counts_need_more_than_32_bits():
    """the chimera at T(c) = 10 F and F in a -m 0 table, the counts raised through
    kc_insert_counts_device (weak_cases.big_counts: products far above 2^32 whose low 32 bits alone give
    the other verdict; T(c) < 2^16 keeps them below 2^64 on any graph a test can hold)"""
    import torch
    seqs, j, f, ratio = wc.big_counts()
    k, W = 31, 1
    with counted_cases(seqs, k, mode=0) as low, fresh(k, 1 << 14, mode=0) as src, fresh(k, 1 << 14, mode=0) as dst:
        n = low.finish()["distinct"]
        buf = torch.zeros(n * (W + 1), dtype=torch.int64, device="cuda")
        assert sum(low.route_table_device(1, buf.data_ptr(), n)) == n
        torch.cuda.synchronize()
        buf.view(-1, W + 1)[:, W] *= f
        torch.cuda.synchronize()
        src.insert_counts_device(buf.data_ptr(), n)
        src.finish()
        table = table_of(src)
        assert table == {c: t * f for c, t in table_of(low).items()} and max(table.values()) == 10 * f
        graph = cm.cdbg(table)
        units, edges, _ = graph
        u = unit_of(units, j, k)
        s, nn = wm.local(units, wm.neighbours(units, edges)[u])
        lhs, rhs = units[u][2] * nn * 1000, ratio * s * units[u][1]
        assert lhs >= 1 << 32 and lhs < rhs and not (lhs & 0xFFFFFFFF < rhs & 0xFFFFFFFF)
        want, st = check_cut(dst, src, table, graph=graph, max_nodes=k, ratio_permille=ratio)
        assert st["cut"] == 1 and set(table) - set(want) == nodes_of(j, k)


# ---- 4. the limits ---------------------------------------------------------------------------------
def test_limits():
    k = 31
    seqs, j = wc.chimera(k)
    with counted_cases(seqs, k, 1 << 15) as src, fresh(k, 1 << 15) as dst:
        table = table_of(src)
        graph = cm.cdbg(table)
        junction = nodes_of(j, k)
        for rule, cut in ((dict(max_nodes=k - 2, ratio_permille=200), 0),  # the joint has k - 1 nodes
                          (dict(max_nodes=k - 1, ratio_permille=200), 1),
                          (dict(), 0),                                      # max_nodes = 0 copies the range
                          (dict(ratio_permille=200, max_mean=5), 0),
                          (dict(max_nodes=k, max_mean=1), 1),               # no relative test: the guard decides
                          (dict(max_nodes=k, ratio_permille=1000), 1),
                          (dict(max_nodes=k, ratio_permille=100), 0),       # 1 is not below a tenth of 10
                          (dict(max_nodes=k, ratio_permille=101), 1)):
            dst.reset()
            want, st = check_cut(dst, src, table, graph=graph, **rule)
            assert st["cut"] == cut and set(table) - set(want) == (junction if cut else set()), rule
            assert st["interior"] == 1 and st["weak"] == (0 if rule.get("ratio_permille") == 100 else 1)
        dst.reset()
        want, st = check_cut(dst, src, table, 2, 0, max_nodes=k, ratio_permille=200)  # the joint is outside the range
        assert set(want) == set(table) - junction and (st["unitigs"], st["interior"]) == (2, 0)
        dst.reset()
        want, st = check_cut(dst, src, table, 1, 1, max_nodes=k, max_mean=1)  # only the joint is in the range: isolated
        assert set(want) == junction and (st["unitigs"], st["interior"], st["cut"]) == (1, 0, 0)


def test_guard_keeps_the_heavier_link():
    """a joint of mean 2 between genomes of mean 10 stays at max_mean = 1 and goes at 2"""
    k = 31
    seqs, j = wc.chimera(k, light=2)
    with counted_cases(seqs, k) as src, fresh(k, 1 << 14) as dst:
        table = table_of(src)
        graph = cm.cdbg(table)
        want, st = check_cut(dst, src, table, graph=graph, max_nodes=k, ratio_permille=500, max_mean=1)
        assert want == table and (st["weak"], st["cut"]) == (1, 0)
        dst.reset()
        want, st = check_cut(dst, src, table, graph=graph, max_nodes=k, ratio_permille=500, max_mean=2)
        assert (st["cut"], st["cut_nodes"]) == (1, k - 1) and all(table[c] == 2 for c in set(table) - set(want))


# ---- 5. what is no weak link stays -----------------------------------------------------------------
def test_what_is_no_weak_link_stays():
    k = 31
    rng = np.random.default_rng(7)
    circle = _bases(rng, 500)
    chain = b">r\n" + _bases(np.random.default_rng(2024), 20000) + b"\n"
    for data, slots in ((cc.fasta(cc.two_tip_junction(k)[0]), 1 << 14), (cc.fasta(cc.cascade(k)[0]), 1 << 14),
                        (cc.fasta(cc.isolated_chain(k)[0]), 1 << 14), (_reads(rng, circle * 3, 400, 100), 1 << 14),
                        (chain, 1 << 16)):
        with count(data, k, table_slots=slots) as src, fresh(k, slots) as dst:
            table = table_of(src)
            want, st = check_cut(dst, src, table, max_nodes=100000, ratio_permille=1000, max_mean=100000)
            assert want == table and (st["cut"], st["out_keys"]) == (0, len(table))


# ---- 6. table states -------------------------------------------------------------------------------
def test_counts_above_the_kaarme_limit():
    """Raw counts move: a k-mer counted 20000 times reads back 16383 from the -m 2 source and 20000 from
    a -m 0 destination, beside a joint that is cut in the same call."""
    k = 31
    seqs, j = wc.chimera(k)
    data = cc.fasta(seqs) + b">a\n" + b"A" * (k - 1 + 20000) + b"\n"
    with count(data, k, mode=2, table_slots=1 << 14) as src, fresh(k, 1 << 14, mode=0) as dst:
        table = table_of(src)
        assert table["A" * k] == 16383
        raw = {"A" * k: 20000}
        want, st = check_cut(dst, src, table, raw=raw, max_nodes=k, ratio_permille=200)
        assert st["cut"] == 1 and want["A" * k] == 20000 and st["out_sum"] == sum(want.values())
        assert int(dst.lookup(ka.encode_kmers(["A" * k], k))[0]) == 20000


def test_results_accumulate_and_drop_the_compact_snapshot(counted):
    k = 31
    kc, table = counted(k)
    graph = counted.model(k)
    with fresh(k) as dst:
        want, st = check_cut(dst, kc, table, graph=graph, max_nodes=2 * k, ratio_permille=500)
        assert st["cut"] > 0 and dst.compact()["kmers"] == len(want)
        total = add_into({}, want)
        want2, st2 = check_cut(dst, kc, table, graph=graph, before=total)  # the rule off: more keys
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
    rule = dict(max_nodes=k, ratio_permille=300, max_mean=40)
    before = (kc.output_digest(), kc.finish())
    want, want_st = wm.cut(table, graph=counted.model(k), **rule)
    assert ka.weak_stats(kc, **rule) == want_st and want_st["cut"] > 0
    d, st = ka.kc_weak_desc(1, 0, k, 300, 40, 0), ka.kc_weak_stats()
    assert kc.lib.kc_cut_weak(None, kc._ctx, ctypes.byref(d), ctypes.byref(st)) == 0 and st.as_dict() == want_st
    assert kc.lib.kc_cut_weak(None, kc._ctx, ctypes.byref(d), None) == 0
    assert kc.lib.kc_cut_weak_device(None, kc._ctx, ctypes.byref(d), None, None) == 0
    assert (kc.output_digest(), kc.finish()) == before
    with fresh(k) as dst:
        was = dst.finish()["inserted"]
        st = dst.cut_weak(kc, **rule)
        assert st == want_st and dst.finish()["inserted"] == was + st["out_sum"]
        assert (kc.output_digest(), kc.finish()) == before
        ok = same(table_of(kc), table)
        assert ok


def test_bloom_gated_source():
    k = 31
    with count(make_reads(5), k, bloom=True, est_unique=150000, fpr=0.01) as src, fresh(k) as dst:
        table = table_of(src)
        assert len(table) > 1000
        _, st = check_cut(dst, src, table, max_nodes=2 * k, ratio_permille=1000)
        assert st["interior"] > 0


def test_full_source_table():
    k = 31
    data = make_reads(40 + k)
    with count(data, k, table_slots=1 << 20) as kc0:
        distinct = kc0.finish()["distinct"]
    with count(data, k, table_slots=distinct) as src, fresh(k) as dst:
        fin = src.finish()
        assert fin["distinct"] == distinct and fin["table_slots"] < 2 * distinct
        table = table_of(src)
        _, st = check_cut(dst, src, table, max_nodes=k, ratio_permille=200)
        assert st["cut"] > 0


def test_emptied_source_adds_nothing():
    k = 31
    data = cc.fasta(wc.chimera(k)[0])
    with count(data, k, table_slots=1 << 15) as src, fresh(k, 1 << 15) as dst:
        assert ka.weak_stats(src, max_nodes=k, ratio_permille=200)["cut"] == 1
        for empty_it in (src.clear_table, src.reset):
            empty_it()
            assert dst.cut_weak(src, max_nodes=k, ratio_permille=200) == ZERO
            assert ka.weak_stats(src) == ZERO and table_of(dst) == {} and dst.finish()["inserted"] == 0
            for off, ln, bh in ka.plan_chunks(data, k, ka.FMT_FASTA):
                src.count_chunk(data[off:off + ln], ka.FMT_FASTA, bool(bh))
            src.finish()


def test_destination_too_small(counted):
    k = 31
    kc, table = counted(k)
    want, want_st = wm.cut(table, graph=counted.model(k), max_nodes=k, ratio_permille=200)
    with fresh(k, slots=64) as tiny:
        assert tiny.finish()["table_slots"] == 4096 < want_st["out_keys"]
        assert tiny.cut_weak(kc, max_nodes=k, ratio_permille=200) == want_st  # the statistics are of the cutting
        with pytest.raises(ka.KcError) as e:
            tiny.finish()
        assert e.value.code == KC_ERR_TABLE_FULL


# ---- 7. rounds: the result is a counted table ------------------------------------------------------
def test_weak_rounds():
    k = 31
    seqs, _ = wc.chimera(k)
    with counted_cases(seqs, k, 1 << 15) as src:
        table = table_of(src)
        rule = dict(max_nodes=k, ratio_permille=200)
        want, want_st = wm.model_rounds(table, 5, **rule)
        assert [s["cut"] for s in want_st] == [1, 0] and want_st[1]["unitigs"] == 2
        out, st = ka.weak_rounds(src, 5, **rule)
        with out:
            assert st == want_st and table_of(out) == want
            assert out.cfg.table_slots == len(want) + len(want) // 8 + 4096
            units, _, cst = check_cdbg(out, want)
            assert cst["nodes"] == len(want) and cst["unitigs"] == 2 and int(out.histogram().sum()) == len(want)
        out, st = ka.weak_rounds(src, 1, **rule)
        with out:
            assert st == want_st[:1] and table_of(out) == want
        assert table_of(src) == table  # the source is not closed and not changed
        with pytest.raises(ValueError):
            ka.weak_rounds(src, 0, **rule)


def test_chain_of_the_three_filters():
    """clean_rounds -> pop_rounds -> weak_rounds, each on the table the one before left, equals the three
    models chained (a quarter of make_reads' genome and reads: the models run five times)"""
    k = 31
    clean_rule = dict(tip_max_nodes=k - 1, iso_max_nodes=k - 1)
    pop_rule = dict(max_nodes=k, max_diff=1)
    weak_rule = dict(max_nodes=2 * k, ratio_permille=300)
    with count(make_reads(k, n_reads=500, genome_len=10000), k, table_slots=1 << 16) as kc:
        table = table_of(kc)
        want1, st1 = clm.model_rounds(table, 1, **clean_rule)
        want2, st2 = bm.model_rounds(want1, 1, **pop_rule)
        want3, st3 = wm.model_rounds(want2, 2, **weak_rule)
        assert st1[0]["tips"] > 0 and st2[0]["popped"] > 0 and st3[0]["cut"] > 0
        cleaned, got1 = ka.clean_rounds(kc, 1, **clean_rule)
        with cleaned:
            popped, got2 = ka.pop_rounds(cleaned, 1, **pop_rule)
            with popped:
                cut, got3 = ka.weak_rounds(popped, 2, **weak_rule)
                with cut:
                    assert (got1, got2, got3) == (st1, st2, st3)
                    ok = same(table_of(cut), want3)
                    assert ok


# ---- 8. ordering -----------------------------------------------------------------------------------
def test_device_form_on_a_side_stream(counted):
    import torch
    k = 31
    kc, table = counted(k)
    rule = dict(max_nodes=k, ratio_permille=200)
    want, want_st = wm.cut(table, graph=counted.model(k), **rule)
    before = (kc.finish(), kc.output_digest())
    with fresh(k) as dst, fresh(k) as host:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            stats = torch.full((8,), -1, dtype=torch.int64, device="cuda")
            dst.cut_weak_device(kc, stats_ptr=stats.data_ptr(), stream=s.cuda_stream, **rule)
            dst.cut_weak_device(kc, stream=s.cuda_stream, **rule)  # (without statistics)
        dst.sync()
        torch.cuda.synchronize()
        assert dict(zip(wm.FIELDS, stats.cpu().tolist())) == want_st == host.cut_weak(kc, **rule)
        ok = same(table_of(dst), add_into(table_of(host), want))
        assert ok
        assert dst.finish()["inserted"] == 2 * want_st["out_sum"]
    assert (kc.finish(), kc.output_digest()) == before


# ---- 9. errors -------------------------------------------------------------------------------------
def test_argument_and_state_errors(counted):
    kc, table = counted(31)
    other_k = counted(32)[0]
    lib = kc.lib

    def rcs(d_, s_, desc):
        """the codes of the host form and of the device form"""
        p = [d_._ctx if d_ else None, s_._ctx if s_ else None, ctypes.byref(desc) if desc else None]
        return lib.kc_cut_weak(*p, None), lib.kc_cut_weak_device(*p, None, None)

    ok = ka.kc_weak_desc(2, 0, 31, 200, 0, 0)
    with fresh(31) as dst:
        assert rcs(dst, kc, ok) == (0, 0)
        filled = table_of(dst)
        arg, state = (KC_ERR_ARG,) * 2, (KC_ERR_STATE,) * 2
        assert rcs(dst, dst, ok) == arg and b"kc_cut_weak: dst must not be src" in lib.kc_last_error(dst._ctx)
        assert rcs(kc, kc, ok) == arg
        assert rcs(dst, other_k, ok) == arg and b"same k" in lib.kc_last_error(dst._ctx)
        assert rcs(dst, kc, ka.kc_weak_desc(2, 0, 31, 200, 0, 1)) == arg and b"reserved" in lib.kc_last_error(dst._ctx)
        assert rcs(dst, kc, ka.kc_weak_desc(3, 2, 31, 200, 0, 0)) == arg and b"min_count" in lib.kc_last_error(dst._ctx)
        # the two of this filter's own
        assert rcs(dst, kc, ka.kc_weak_desc(2, 0, 31, 1001, 0, 0)) == arg
        assert b"kc_cut_weak: ratio_permille must be at most 1000" in lib.kc_last_error(dst._ctx)
        assert rcs(dst, kc, ka.kc_weak_desc(2, 0, 31, 0, 0, 0)) == arg
        assert b"kc_cut_weak: max_nodes needs ratio_permille or max_mean" in lib.kc_last_error(dst._ctx)
        assert rcs(None, kc, ka.kc_weak_desc(2, 0, 31, 1001, 0, 0)) == arg and b"ratio_permille" in lib.kc_last_error(kc._ctx)
        assert rcs(dst, kc, ka.kc_weak_desc(3, 3, 31, 1000, 0, 0)) == (0, 0)
        once = wm.cut(table, 3, 3, max_nodes=31, ratio_permille=1000)[0]
        filled = add_into(add_into(filled, once), once)
        assert rcs(dst, kc, ka.kc_weak_desc(3, 3, 0, 0, 0, 0)) == (0, 0)  # max_nodes = 0: nothing to refuse
        once = wm.cut(table, 3, 3)[0]
        filled = add_into(add_into(filled, once), once)
        assert rcs(dst, None, ok) == arg and rcs(dst, kc, None) == arg and rcs(None, None, ok) == arg
        assert b"kc_cut_weak: null source or descriptor" in lib.kc_last_error(dst._ctx)
        # without dst the message is on src
        assert rcs(None, kc, ka.kc_weak_desc(3, 2, 0, 0, 0, 0)) == arg and b"min_count" in lib.kc_last_error(kc._ctx)
        with pytest.raises(ka.KcError) as e:
            dst.cut_weak(kc, 5, 4)
        assert e.value.code == KC_ERR_ARG and "min_count" in str(e.value)
        with pytest.raises(ka.KcError) as e:
            dst.cut_weak(kc, max_nodes=31)
        assert e.value.code == KC_ERR_ARG and "max_nodes needs" in str(e.value)
        # k < 2
        with count(b">t\nACGTTGCA\n", 1, table_slots=1 << 12) as k1, fresh(1, 1 << 12) as d1:
            assert rcs(d1, k1, ka.kc_weak_desc(1, 0, 0, 0, 0, 0)) == arg and rcs(None, k1, ok) == arg
        # a Bloom context has no table before kc_bloom_finalize: as src and as dst
        with ka.KmerCounter(ka.Config(k=31, bf_enable=True, est_unique=100000, min_abundance=1)) as nb:
            assert rcs(dst, nb, ok) == state and rcs(None, nb, ok) == state and rcs(nb, kc, ok) == state
            assert b"a weak-link removal" in lib.kc_last_error(nb._ctx)
        # none of the refused calls changed dst
        ok_ = same(table_of(dst), filled)
        assert ok_
        assert dst.finish()["inserted"] == sum(filled.values())
