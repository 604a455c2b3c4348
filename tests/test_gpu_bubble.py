"""GPU: bubble popping (kc_pop_bubbles*; KmerCounter.pop_bubbles / pop_bubbles_device, bubble_stats,
pop_rounds) against the pure-Python model bubble_model.py applied to the source table's own dump().

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
import graph_model as m
import kaarme_amd as ka
from test_gpu_cdbg import check_cdbg
from test_gpu_clean import add_into, fresh
from test_gpu_graph import _bases, _reads, count, make_reads, same, table_of
from test_gpu_unitig import HAIR

pytestmark = pytest.mark.gpu

KC_ERR_ARG, KC_ERR_TABLE_FULL, KC_ERR_STATE = -1, -3, -4
KS = [15, 31, 32, 63, 65, 479]
READ_KS = [15, 31, 32]
ZERO = dict.fromkeys(bm.FIELDS, 0)


# ---- helpers ---------------------------------------------------------------------------------------
def check_pop(dst, src, table, lo=1, hi=0, graph=None, raw=None, before=None, **rule):
    """dst (holding `before`, default nothing) after dst.pop_bubbles(src, lo, hi, **rule) == the model on
    the table; returns (the model's kept table, the statistics)"""
    want, want_st = bm.pop(table, lo, hi, raw=raw, graph=graph, **rule)
    st = dst.pop_bubbles(src, lo, hi, **rule)
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


@pytest.mark.parametrize("k", _widths())
def test_every_key_width(k):
    seqs, _ = bc.variants(k)
    with counted_cases(seqs, k, 1 << 15) as src, fresh(k, 1 << 17) as dst:
        assert dst.finish()["table_slots"] != src.finish()["table_slots"]  # the keys move between two geometries
        table = table_of(src)
        for lo, hi in ((1, 0), (2, 0)):
            graph = cm.cdbg(table, lo, hi)
            rule = dict(max_nodes=k, max_diff=1)
            want, want_st = bm.pop(table, lo, hi, graph=graph, **rule)
            if lo == 1:
                assert (want_st["unitigs"], want_st["branches"], want_st["parallel"], want_st["popped"]) == (14, 9, 9, 5)
            else:  # the variants are given once: from T(c) >= 2 on the genome is one chain
                assert (want_st["unitigs"], want_st["branches"], want_st["popped"]) == (1, 0, 0)
            dst.reset()
            check_pop(dst, src, table, lo, hi, graph=graph, **rule)
            assert ka.bubble_stats(src, lo, hi, **rule) == want_st
            assert dst.finish()["inserted"] == want_st["out_sum"]


# ---- 2. real read errors ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", READ_KS)
def test_read_errors(k, counted):
    kc, table = counted(k)
    graph = counted.model(k)
    with fresh(k) as dst:
        want, st = check_pop(dst, kc, table, graph=graph, max_nodes=k, max_diff=0)
        assert st["popped"] > 0 and st["parallel"] >= 2 * st["popped"] > 0 and st["branches"] > st["parallel"]
        dst.reset()
        _, st1 = check_pop(dst, kc, table, graph=graph, max_nodes=k, max_diff=1)
        assert st1["popped"] >= st["popped"]


# ---- 3. the bubble of clean_cases ------------------------------------------------------------------
def test_bubble_loses_the_substituted_arm():
    k = 31
    (g0, alt), q = cc.bubble(k)
    arm = {m.canon(alt[i:i + k]) for i in range(len(alt) - k + 1)} - {m.canon(g0[i:i + k]) for i in range(len(g0) - k + 1)}
    assert len(arm) == k
    with counted_cases([g0] * 3 + [alt], k) as src, fresh(k, 1 << 14) as dst:
        table = table_of(src)
        want, st = check_pop(dst, src, table, max_nodes=k)
        assert set(table) - set(want) == arm and (st["branches"], st["parallel"], st["popped"], st["popped_nodes"]) == (2, 2, 1, k)
        dst.finish()
        units, _, cst = check_cdbg(dst, want)
        assert [(u[1], u[3]) for u in units] == [(100, False)]
    # given once each, the means are equal: the same arm goes whichever sequence comes first
    gone = []
    for seqs in ([g0, alt], [alt, g0]):
        with counted_cases(seqs, k) as src, fresh(k, 1 << 14) as dst:
            table = table_of(src)
            want, st = check_pop(dst, src, table, max_nodes=k)
            assert st["popped"] == 1 and len(want) == 100
            gone.append(frozenset(set(table) - set(want)))
    assert gone[0] == gone[1]


# ---- 4. the limits ---------------------------------------------------------------------------------
def test_limits():
    k = 31
    seqs, alts = bc.variants(k)
    g_nodes = {m.canon(seqs[0][i:i + k]) for i in range(len(seqs[0]) - k + 1)}
    dele = next(a for _, kind, a in alts if kind == "del")
    del_nodes = {m.canon(dele[i:i + k]) for i in range(len(dele) - k + 1)} - g_nodes
    assert len(del_nodes) == k - 1
    with counted_cases(seqs, k, 1 << 15) as src, fresh(k, 1 << 15) as dst:
        table = table_of(src)
        graph = cm.cdbg(table)
        want, st = check_pop(dst, src, table, graph=graph, max_nodes=k - 1)
        assert want == table and (st["parallel"], st["popped"]) == (9, 0)
        dst.reset()
        want, st = check_pop(dst, src, table, graph=graph, max_nodes=k - 1, max_diff=1)  # the deletion's arm fits, the genome's not
        assert want == table and st["popped"] == 0
        dst.reset()
        want, st = check_pop(dst, src, table, graph=graph)  # max_nodes = 0 copies the range
        assert want == table and (st["branches"], st["parallel"], st["popped"], st["out_keys"]) == (9, 9, 0, len(table))
        dst.reset()
        want, st = check_pop(dst, src, table, graph=graph, max_nodes=k)
        assert st["popped"] == 4 and del_nodes <= set(want)
        dst.reset()
        want, st = check_pop(dst, src, table, graph=graph, max_nodes=k, max_diff=1)
        assert st["popped"] == 5 and set(want) == g_nodes
        dst.reset()
        want, st = check_pop(dst, src, table, 2, 0, max_nodes=k, max_diff=1)  # the variants are outside the range
        assert set(want) == g_nodes and (st["unitigs"], st["branches"]) == (1, 0)


def test_guard_keeps_the_heavier_arm():
    """an arm of mean 2 beside one of mean 6 stays at max_mean = 1 and goes at 2"""
    k = 31
    seqs, alts = bc.variants(k, heavy=6, sites=1)
    alt = alts[0][2]
    with counted_cases(seqs + [alt], k) as src, fresh(k, 1 << 14) as dst:
        table = table_of(src)
        graph = cm.cdbg(table)
        units, edges, _ = graph
        arms = sorted((units[u][2], units[u][1]) for u in bm.branches(units, edges))
        assert arms == [(2 * k, k), (6 * k, k)]
        want, st = check_pop(dst, src, table, graph=graph, max_nodes=k, max_mean=1)
        assert want == table and (st["parallel"], st["popped"]) == (2, 0)
        dst.reset()
        want, st = check_pop(dst, src, table, graph=graph, max_nodes=k, max_mean=2)
        assert (st["popped"], st["popped_nodes"]) == (1, k) and all(table[c] == 2 for c in set(table) - set(want))


# ---- 5. what is no bubble stays --------------------------------------------------------------------
def test_what_is_no_bubble_stays():
    k = 31
    rng = np.random.default_rng(7)
    circle = _bases(rng, 500)
    hair = (">a\n" + "A" * 60 + "\n>ca\n" + "CA" * 40 + "\n>h\n" + HAIR + m.rc(HAIR) + "\n").encode()
    chain = b">r\n" + _bases(np.random.default_rng(2024), 20000) + b"\n"
    for data, slots in ((cc.fasta(cc.two_tip_junction(k)[0]), 1 << 14), (hair, 1 << 14),
                        (_reads(rng, circle * 3, 400, 100), 1 << 14), (chain, 1 << 16)):
        with count(data, k, table_slots=slots) as src, fresh(k, slots) as dst:
            table = table_of(src)
            want, st = check_pop(dst, src, table, max_nodes=100000, max_diff=100000)
            assert want == table and (st["parallel"], st["popped"], st["out_keys"]) == (0, 0, len(table))


# ---- 6. dense small k, palindromic anchors ---------------------------------------------------------
@pytest.mark.parametrize("k,length,sites,seeds", [(6, 100, 8, (130, 160, 0, 1, 2, 3)), (8, 400, 20, (21, 0, 1))])
def test_dense_small_k(k, length, sites, seeds):
    """accidental repeats, self loops and palindromic nodes; the first seed has a set of parallel branches
    one of whose anchors is a palindromic unitig (found by a search on the model)"""
    popped = 0
    with fresh(k, 1 << 14) as dst:
        for n, seed in enumerate(seeds):
            with counted_cases(bc.dense(k, seed, length, sites), k) as src:
                table = table_of(src)
                for lo in (1, 2):
                    graph = cm.cdbg(table, lo, 0)
                    if n == 0 and lo == 1:
                        units, edges, _ = graph
                        br = bm.branches(units, edges)
                        twice = {a for a in br.values() if list(br.values()).count(a) > 1}
                        assert any(units[v][0] == m.rc(units[v][0]) for a in twice for v, _ in a)
                    for rule in (dict(max_nodes=k), dict(max_nodes=k, max_diff=1), dict(max_nodes=3 * k, max_diff=k, max_mean=2)):
                        dst.reset()
                        popped += check_pop(dst, src, table, lo, 0, graph=graph, **rule)[1]["popped"]
    assert popped > 0


@pytest.mark.parametrize("k", [6, 32])
def test_palindromic_anchor(k):
    seqs, p = bc.palindromic_anchor(k)
    with counted_cases(seqs, k) as src, fresh(k, 1 << 14) as dst:
        table = table_of(src)
        assert p == m.rc(p) and p in table
        want, st = check_pop(dst, src, table, max_nodes=k)
        assert (st["branches"], st["parallel"], st["popped"], st["popped_nodes"]) == (2, 2, 1, k) and p in want


# ---- 7. table states -------------------------------------------------------------------------------
def test_counts_above_the_kaarme_limit():
    """Raw counts move: a k-mer counted 20000 times reads back 16383 from the -m 2 source and 20000 from
    a -m 0 destination, beside a bubble that is popped in the same call."""
    k = 31
    seqs, alts = bc.variants(k, sites=1, heavy=1)
    g0 = seqs[0]
    data = cc.fasta(seqs) + b">a\n" + b"A" * (k - 1 + 20000) + g0[:60].encode() + b"\n"
    with count(data, k, mode=2, table_slots=1 << 14) as src, fresh(k, 1 << 14, mode=0) as dst:
        table = table_of(src)
        assert table["A" * k] == 16383
        raw = {"A" * k: 20000}
        want, st = check_pop(dst, src, table, raw=raw, max_nodes=k)
        assert st["popped"] == 1 and want["A" * k] == 20000 and st["out_sum"] == sum(want.values())
        assert int(dst.lookup(ka.encode_kmers(["A" * k], k))[0]) == 20000


def test_results_accumulate_and_drop_the_compact_snapshot(counted):
    k = 31
    kc, table = counted(k)
    graph = counted.model(k)
    with fresh(k) as dst:
        want, st = check_pop(dst, kc, table, graph=graph, max_nodes=k, max_diff=1)
        assert st["popped"] > 0 and dst.compact()["kmers"] == len(want)
        total = add_into({}, want)
        want2, st2 = check_pop(dst, kc, table, graph=graph, before=total)  # the rule off: more keys
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
    rule = dict(max_nodes=k, max_diff=1, max_mean=40)
    before = (kc.output_digest(), kc.finish())
    want, want_st = bm.pop(table, graph=counted.model(k), **rule)
    assert ka.bubble_stats(kc, **rule) == want_st and want_st["popped"] > 0
    d, st = ka.kc_bubble_desc(1, 0, k, 1, 40, 0), ka.kc_bubble_stats()
    assert kc.lib.kc_pop_bubbles(None, kc._ctx, ctypes.byref(d), ctypes.byref(st)) == 0 and st.as_dict() == want_st
    assert kc.lib.kc_pop_bubbles(None, kc._ctx, ctypes.byref(d), None) == 0
    assert kc.lib.kc_pop_bubbles_device(None, kc._ctx, ctypes.byref(d), None, None) == 0
    assert (kc.output_digest(), kc.finish()) == before
    with fresh(k) as dst:
        was = dst.finish()["inserted"]
        st = dst.pop_bubbles(kc, **rule)
        assert st == want_st and dst.finish()["inserted"] == was + st["out_sum"]
        assert (kc.output_digest(), kc.finish()) == before
        ok = same(table_of(kc), table)
        assert ok


def test_bloom_gated_source():
    k = 31
    with count(make_reads(5), k, bloom=True, est_unique=150000, fpr=0.01) as src, fresh(k) as dst:
        table = table_of(src)
        assert len(table) > 1000
        _, st = check_pop(dst, src, table, max_nodes=k, max_diff=1)
        assert st["branches"] > 0


def test_full_source_table():
    k = 31
    data = make_reads(40 + k)
    with count(data, k, table_slots=1 << 20) as kc0:
        distinct = kc0.finish()["distinct"]
    with count(data, k, table_slots=distinct) as src, fresh(k) as dst:
        fin = src.finish()
        assert fin["distinct"] == distinct and fin["table_slots"] < 2 * distinct
        table = table_of(src)
        _, st = check_pop(dst, src, table, max_nodes=k, max_diff=1)
        assert st["popped"] > 0


def test_emptied_source_adds_nothing():
    k = 31
    data = cc.fasta(bc.variants(k)[0])
    with count(data, k, table_slots=1 << 15) as src, fresh(k, 1 << 15) as dst:
        assert ka.bubble_stats(src, max_nodes=k)["popped"] == 4
        for empty_it in (src.clear_table, src.reset):
            empty_it()
            assert dst.pop_bubbles(src, max_nodes=k, max_diff=1) == ZERO
            assert ka.bubble_stats(src) == ZERO and table_of(dst) == {} and dst.finish()["inserted"] == 0
            for off, ln, bh in ka.plan_chunks(data, k, ka.FMT_FASTA):
                src.count_chunk(data[off:off + ln], ka.FMT_FASTA, bool(bh))
            src.finish()


def test_destination_too_small(counted):
    k = 31
    kc, table = counted(k)
    want, want_st = bm.pop(table, graph=counted.model(k), max_nodes=k)
    with fresh(k, slots=64) as tiny:
        assert tiny.finish()["table_slots"] == 4096 < want_st["out_keys"]
        assert tiny.pop_bubbles(kc, max_nodes=k) == want_st  # the statistics are of the popping
        with pytest.raises(ka.KcError) as e:
            tiny.finish()
        assert e.value.code == KC_ERR_TABLE_FULL


# ---- 8. rounds: the result is a counted table ------------------------------------------------------
def test_pop_rounds():
    k = 31
    seqs, _ = bc.variants(k)
    with counted_cases(seqs, k, 1 << 15) as src:
        table = table_of(src)
        want, want_st = bm.model_rounds(table, 5, max_nodes=k, max_diff=1)
        assert [s["popped"] for s in want_st] == [5, 0] and want_st[1]["unitigs"] == 1
        out, st = ka.pop_rounds(src, 5, max_nodes=k, max_diff=1)
        with out:
            assert st == want_st and table_of(out) == want
            assert out.cfg.table_slots == len(want) + len(want) // 8 + 4096
            units, _, cst = check_cdbg(out, want)
            assert cst["nodes"] == len(want) and cst["unitigs"] == 1 and int(out.histogram().sum()) == len(want)
        out, st = ka.pop_rounds(src, 1, max_nodes=k, max_diff=1)
        with out:
            assert st == want_st[:1] and table_of(out) == want
        assert table_of(src) == table  # the source is not closed and not changed
        with pytest.raises(ValueError):
            ka.pop_rounds(src, 0, max_nodes=k)


# ---- 9. ordering -----------------------------------------------------------------------------------
def test_device_form_on_a_side_stream(counted):
    import torch
    k = 31
    kc, table = counted(k)
    rule = dict(max_nodes=k, max_diff=1)
    want, want_st = bm.pop(table, graph=counted.model(k), **rule)
    before = (kc.finish(), kc.output_digest())
    with fresh(k) as dst:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            stats = torch.full((8,), -1, dtype=torch.int64, device="cuda")
            dst.pop_bubbles_device(kc, stats_ptr=stats.data_ptr(), stream=s.cuda_stream, **rule)
            dst.pop_bubbles_device(kc, stream=s.cuda_stream, **rule)  # (without statistics)
        dst.sync()
        torch.cuda.synchronize()
        assert dict(zip(bm.FIELDS, stats.cpu().tolist())) == want_st
        ok = same(table_of(dst), add_into(dict(want), want))
        assert ok
        assert dst.finish()["inserted"] == 2 * want_st["out_sum"]
    assert (kc.finish(), kc.output_digest()) == before


# ---- 10. errors ------------------------------------------------------------------------------------
def test_argument_and_state_errors(counted):
    kc, table = counted(31)
    other_k = counted(32)[0]
    lib = kc.lib

    def rcs(d_, s_, desc):
        """the codes of the host form and of the device form"""
        p = [d_._ctx if d_ else None, s_._ctx if s_ else None, ctypes.byref(desc) if desc else None]
        return lib.kc_pop_bubbles(*p, None), lib.kc_pop_bubbles_device(*p, None, None)

    ok = ka.kc_bubble_desc(2, 0, 31, 1, 0, 0)
    with fresh(31) as dst:
        assert rcs(dst, kc, ok) == (0, 0)
        filled = table_of(dst)
        arg, state = (KC_ERR_ARG,) * 2, (KC_ERR_STATE,) * 2
        assert rcs(dst, dst, ok) == arg and b"kc_pop_bubbles: dst must not be src" in lib.kc_last_error(dst._ctx)
        assert rcs(kc, kc, ok) == arg
        assert rcs(dst, other_k, ok) == arg and b"same k" in lib.kc_last_error(dst._ctx)
        assert rcs(dst, kc, ka.kc_bubble_desc(2, 0, 31, 1, 0, 1)) == arg and b"reserved" in lib.kc_last_error(dst._ctx)
        assert rcs(dst, kc, ka.kc_bubble_desc(3, 2, 31, 1, 0, 0)) == arg and b"min_count" in lib.kc_last_error(dst._ctx)
        assert rcs(dst, kc, ka.kc_bubble_desc(3, 3, 31, 1, 0, 0)) == (0, 0)
        once = bm.pop(table, 3, 3, max_nodes=31, max_diff=1)[0]
        filled = add_into(add_into(filled, once), once)
        assert rcs(dst, None, ok) == arg and rcs(dst, kc, None) == arg and rcs(None, None, ok) == arg
        assert b"kc_pop_bubbles: null source or descriptor" in lib.kc_last_error(dst._ctx)
        # without dst the message is on src
        assert rcs(None, kc, ka.kc_bubble_desc(3, 2, 0, 0, 0, 0)) == arg and b"min_count" in lib.kc_last_error(kc._ctx)
        with pytest.raises(ka.KcError) as e:
            dst.pop_bubbles(kc, 5, 4)
        assert e.value.code == KC_ERR_ARG and "min_count" in str(e.value)
        # k < 2
        with count(b">t\nACGTTGCA\n", 1, table_slots=1 << 12) as k1, fresh(1, 1 << 12) as d1:
            assert rcs(d1, k1, ka.kc_bubble_desc(1, 0, 0, 0, 0, 0)) == arg and rcs(None, k1, ok) == arg
        # a Bloom context has no table before kc_bloom_finalize: as src and as dst
        with ka.KmerCounter(ka.Config(k=31, bf_enable=True, est_unique=100000, min_abundance=1)) as nb:
            assert rcs(dst, nb, ok) == state and rcs(None, nb, ok) == state and rcs(nb, kc, ok) == state
        # none of the refused calls changed dst
        ok_ = same(table_of(dst), filled)
        assert ok_
        assert dst.finish()["inserted"] == sum(filled.values())
