"""GPU: the compacted de Bruijn graph of the counted table (kc_unitig_graph*; KmerCounter.unitig_graph
/ unitig_graph_stats / unitig_graph_device) against the pure-Python model cdbg_model.py applied to
the table's own dump().

Expected = the model on decode_records(dump()); actual = the device's records, bases and edges.
Strand, start and order are unspecified, so the unitigs are compared as the sorted list of (normal,
n_nodes, count_sum, circular) and the edges as cdbg_model.normalised_edges, both exactly.  Every case
first checks on the model that its input holds what it claims to exercise."""
import ctypes

import numpy as np
import pytest

import cdbg_model as cm
import graph_model as m
import kaarme_amd as ka
import unitig_model as um
from test_gpu_graph import _bases, _reads, count, make_reads, table_of
from test_gpu_unitig import units_of, wide_reads

pytestmark = pytest.mark.gpu

KC_ERR_ARG, KC_ERR_STATE = -1, -4
KS = [15, 31, 32, 63, 65, 479]
RANGES = [(1, 0), (2, 0), (2, 50)]
STAT_FIELDS = ("unitigs", "circular", "nodes", "bases", "max_nodes", "edges", "dead_ends")
SENT32 = 0x5A5A5A5A


# ---- helpers ---------------------------------------------------------------------------------------
def check_cdbg(kc, table, lo=1, hi=0, want=None):
    """kc.unitig_graph(lo, hi) and kc.unitig_graph_stats(lo, hi) == the model on the table, and the
    edge count follows from kc.graph_stats; returns the model's (units, edges, stats)"""
    k = kc.cfg.k
    units, edges, st = want or cm.cdbg(table, lo, hi)
    records, bases, got_e, got_st = kc.unitig_graph(lo, hi)
    assert got_st == st, (lo, hi, got_st, st)
    assert records.shape == (st["unitigs"], 4) and bases.shape == (st["bases"],) and got_e.shape == (st["edges"],)
    got_units = units_of(records, bases, k, st["bases"])
    um.check_strings(got_units, k)
    assert um.normalised(got_units) == um.normalised(units), (lo, hi)
    tuples = cm.edge_tuples(got_e)
    assert all(a < st["unitigs"] and b < st["unitigs"] for a, _, b, _ in tuples)
    assert cm.normalised_edges(got_units, tuples) == cm.normalised_edges(units, edges), (lo, hi)
    assert kc.unitig_graph_stats(lo, hi) == st
    gst = kc.graph_stats(lo, hi)
    assert st["edges"] == gst["edge_ends"] - gst["link_ends"] - cm.palindromic_left_ends(table, lo, hi)
    return units, edges, st


def self_mirrors(edges):
    """the hairpins (U, a, U, !a)"""
    return [e for e in edges if e[0] == e[2] and e[1] != e[3]]


@pytest.fixture(scope="module")
def counted():
    """k -> (counter, its table as a dict), made once; .model(k, lo, hi) -> the model's graph, made once"""
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
    want = counted.model(k, lo, hi)
    units, edges, st = want
    assert st["nodes"] > st["unitigs"] > 1
    if (lo, hi) == (1, 0):
        assert st["edges"] > 0 and st["dead_ends"] > 0
        if k == 15:
            assert len(self_mirrors(edges)) >= 1
    check_cdbg(kc, table, lo, hi, want=want)


# ---- 2. dense small k ------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n", [(4, 300), (6, 3000)])
def test_dense_small_k(k, n):
    """palindromic nodes with neighbours, self loops and sides of degree 4"""
    rng = np.random.default_rng(200 + k)
    with count(b">t\n" + _bases(rng, n) + b"\n", k, table_slots=1 << 14) as kc:
        table = table_of(kc)
        med = int(np.median(list(table.values())))
        nodes = set(table)
        pals = [c for c in nodes if c == m.rc(c)]
        assert any(m.edge_info(nodes, c)[0] for c in pals)
        assert m.graph(table)[1]["side_degree"][4] > 0
        units, edges, st = check_cdbg(kc, table)
        assert any(e[0] == e[2] for e in edges) and cm.palindromic_left_ends(table) > 0
        check_cdbg(kc, table, med, 0)
        check_cdbg(kc, table, 1, med)


# ---- 3. one long chain -----------------------------------------------------------------------------
def test_one_long_chain():
    k = 31
    rng = np.random.default_rng(2024)
    read = _bases(rng, 20000)
    with count(b">r\n" + read + b"\n", k, table_slots=1 << 16) as kc:
        table = table_of(kc)
        want = cm.cdbg(table)
        assert [(u[1], u[3]) for u in want[0]] == [(20000 - k + 1, False)] and want[1] == []
        assert (want[2]["edges"], want[2]["dead_ends"]) == (0, 2)
        check_cdbg(kc, table, want=want)


# ---- 4. a circle -----------------------------------------------------------------------------------
def test_circle_of_500_nodes():
    k = 31
    rng = np.random.default_rng(7)
    circle = _bases(rng, 500)
    with count(_reads(rng, circle * 3, 400, 100), k, table_slots=1 << 14) as kc:
        table = table_of(kc)
        want = cm.cdbg(table)
        assert [(u[1], u[3]) for u in want[0]] == [(500, True)] and want[1] == []
        assert (want[2]["circular"], want[2]["edges"], want[2]["dead_ends"]) == (1, 0, 0)
        check_cdbg(kc, table, want=want)
        records, bases, edges, st = kc.unitig_graph()
        lines = ka.gfa_lines(records, bases, edges, k)
        assert len(lines) == 4 and lines[0] == "H\tVN:Z:1.0" and lines[1].startswith("S\t0\t")
        assert lines[1].endswith(f"\tLN:i:{500 + k - 1}\tKC:i:{want[0][0][2]}")
        assert lines[2:] == ["L\t0\t+\t0\t+\t30M", "L\t0\t-\t0\t-\t30M"]


# ---- 5. capacities ---------------------------------------------------------------------------------
def _device_call(kc, lo, hi, cap_u, cap_b, cap_e, guard=16, **kw):
    """unitig_graph_device into sentinel-filled buffers of the capacities plus a guard; the host copies"""
    import torch
    recs = torch.full(((cap_u + guard) * 4,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    bases = torch.full((cap_b + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    edges = torch.full(((cap_e + guard) * 4,), SENT32, dtype=torch.int32, device="cuda")
    stats = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    kc.unitig_graph_device(lo, hi, recs.data_ptr(), cap_u, bases.data_ptr(), cap_b, edges.data_ptr(), cap_e,
                           stats.data_ptr(), **kw)
    torch.cuda.synchronize()
    return (recs.cpu().numpy().view(np.uint64), bases.cpu().numpy(), edges.cpu().numpy().view(np.uint32),
            stats.cpu().tolist())


def test_capacities_bound_the_edges(counted):
    import torch
    k, lo, hi = 31, 2, 0
    kc, table = counted(k)
    units, edges, st = counted.model(k, lo, hi)
    want_e = cm.normalised_edges(units, edges)
    n, nb, ne = st["unitigs"], st["bases"], st["edges"]
    totals = [st[f] for f in STAT_FIELDS] + [0]
    assert ne > 2 and n > 4
    # statistics only: the full totals without any buffer
    stats = torch.full((8,), -1, dtype=torch.int64, device="cuda")
    kc.unitig_graph_device(lo, hi, stats_ptr=stats.data_ptr())
    kc.unitig_graph_device(lo, hi, 0, 1 << 40, 0, 1 << 40, 0, 1 << 40, 0)  # (capacities without buffers are not used)
    kc.unitig_graph_device(lo, hi)
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == totals
    for cap_e in (0, 1, ne - 1, ne):
        hr, hb, he, hs = _device_call(kc, lo, hi, n, nb, cap_e)
        assert hs == totals  # the totals are always full
        assert (he[cap_e * 4:] == SENT32).all() and (hr[n * 4:] == np.uint64(0x5A5A5A5A5A5A5A5A)).all()
        written = he[:min(cap_e, ne) * 4]
        assert not (written.reshape(-1, 4)[:, :2] == SENT32).any()  # exactly min(cap, total) records are written
        got_units = units_of(hr[:n * 4], hb, k, nb)
        got = cm.normalised_edges(got_units, cm.edge_tuples(written.view(ka.EDGE_DTYPE)))
        assert len(got) == min(cap_e, ne) and len(set(got)) == len(got) and set(got) <= set(want_e)
        if cap_e == ne:
            assert got == want_e
    # fewer unitig records than unitigs: the edges are still complete and number the unitigs there are
    cap_u = n // 2
    hr, hb, he, hs = _device_call(kc, lo, hi, cap_u, nb, ne)
    assert hs == totals and (hr[cap_u * 4:] == np.uint64(0x5A5A5A5A5A5A5A5A)).all() and (he[ne * 4:] == SENT32).all()
    tuples = cm.edge_tuples(he[:ne * 4].view(ka.EDGE_DTYPE))
    assert len(tuples) == ne == len(set(tuples)) and all(a < n and b < n for a, _, b, _ in tuples)
    # the edges between the unitigs whose records were written are the model's between those
    got_units = units_of(hr[:cap_u * 4], hb, k)
    names = {u[0] for u in um.normalised(got_units)}
    inner = [e for e in tuples if e[0] < cap_u and e[2] < cap_u]
    assert inner and cm.normalised_edges(got_units, inner) == [e for e in want_e if e[0] in names and e[2] in names]


# ---- 6. ordering -----------------------------------------------------------------------------------
def test_device_form_on_a_side_stream(counted):
    import torch
    k = 31
    kc, table = counted(k)
    units, edges, st = counted.model(k)
    before = (kc.finish(), table_of(kc))
    n, nb, ne = st["unitigs"], st["bases"], st["edges"]
    src = torch.full((ne * 4,), SENT32, dtype=torch.int32).pin_memory()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev_e = torch.empty(ne * 4, dtype=torch.int32, device="cuda")
        dev_e.copy_(src, non_blocking=True)  # the call's writes follow this copy on the stream
        recs = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        bases = torch.zeros(nb, dtype=torch.uint8, device="cuda")
        stats = torch.full((8,), -1, dtype=torch.int64, device="cuda")
        kc.unitig_graph_device(1, 0, recs.data_ptr(), n, bases.data_ptr(), nb, dev_e.data_ptr(), ne, stats.data_ptr(),
                               stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert stats.cpu().tolist() == [st[f] for f in STAT_FIELDS] + [0]
    got_units = units_of(recs.cpu().numpy().view(np.uint64), bases.cpu().numpy(), k, nb)
    assert um.normalised(got_units) == um.normalised(units)
    got_e = cm.edge_tuples(dev_e.cpu().numpy().view(np.uint32).view(ka.EDGE_DTYPE))
    assert cm.normalised_edges(got_units, got_e) == cm.normalised_edges(units, edges)
    # the table is only read: no counter moved, the dump is the same
    assert kc.finish() == before[0] and table_of(kc) == before[1]


# ---- 7. errors and states --------------------------------------------------------------------------
def test_argument_and_state_errors(counted):
    import torch
    kc, table = counted(31)
    lib = kc.lib
    st = ka.kc_cdbg_stats()
    assert lib.kc_unitig_graph(kc._ctx, 3, 2, None, None, None, ctypes.byref(st)) == KC_ERR_ARG
    assert lib.kc_unitig_graph_device(kc._ctx, 3, 2, None, 0, None, 0, None, 0, None, None) == KC_ERR_ARG
    assert lib.kc_unitig_graph(kc._ctx, 3, 3, None, None, None, ctypes.byref(st)) == 0
    assert st.nodes == sum(1 for t in table.values() if t == 3) and st.reserved == 0
    with pytest.raises(ka.KcError) as e:
        kc.unitig_graph(5, 4)
    assert e.value.code == KC_ERR_ARG and "min_count" in str(e.value)
    buf = torch.zeros(64, dtype=torch.int32, device="cuda")
    with pytest.raises(ka.KcError) as e:  # an edge is one 16-byte store
        kc.unitig_graph_device(1, 0, edges_ptr=buf.data_ptr() + 4, cap_edges=1)
    assert e.value.code == KC_ERR_ARG and "aligned" in str(e.value)
    with ka.KmerCounter(ka.Config(k=31, bf_enable=True, est_unique=100000, min_abundance=1)) as nb:
        assert lib.kc_unitig_graph(nb._ctx, 1, 0, None, None, None, ctypes.byref(st)) == KC_ERR_STATE
        assert lib.kc_unitig_graph_device(nb._ctx, 1, 0, None, 0, None, 0, None, 0, None, None) == KC_ERR_STATE
    with count(b">t\nACGTTGCA\n", 1, table_slots=1 << 12) as k1:
        assert lib.kc_unitig_graph(k1._ctx, 1, 0, None, None, None, ctypes.byref(st)) == KC_ERR_ARG
        assert lib.kc_unitig_graph_device(k1._ctx, 1, 0, None, 0, None, 0, None, 0, None, None) == KC_ERR_ARG


def test_emptied_table_has_no_graph(counted):
    k = 31
    data = make_reads(k)
    units, edges, st = counted.model(k)
    zero = dict.fromkeys(STAT_FIELDS, 0)
    with count(data, k) as kc:
        check_cdbg(kc, counted(k)[1], want=(units, edges, st))
        for empty_it in (kc.clear_table, kc.reset):
            empty_it()
            records, bases, got_e, got_st = kc.unitig_graph()
            assert records.shape == (0, 4) and bases.shape == (0,) and got_e.shape == (0,) and got_st == zero
            assert kc.unitig_graph_stats() == zero
            for off, ln, bh in ka.plan_chunks(data, k, ka.FMT_FASTA):
                kc.count_chunk(data[off:off + ln], ka.FMT_FASTA, bool(bh))
            kc.finish()
            assert kc.unitig_graph_stats() == st


# ---- 8. kc_unitigs is not disturbed ----------------------------------------------------------------
def test_does_not_disturb_unitigs(counted):
    k = 31
    kc, table = counted(k)
    fin = kc.finish()
    before = kc.unitigs()
    records, bases, edges, st = kc.unitig_graph()
    after = kc.unitigs()
    assert before[2] == after[2] == {f: st[f] for f in STAT_FIELDS[:5]}
    assert um.normalised(units_of(*before[:2], k)) == um.normalised(units_of(*after[:2], k)) \
        == um.normalised(units_of(records, bases, k))
    assert kc.finish() == fin
