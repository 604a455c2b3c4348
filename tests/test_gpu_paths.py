"""GPU: read paths through the compacted graph (kc_read_paths*; KmerCounter.read_paths /
read_path_stats / read_paths_device) against the pure-Python model path_model.py applied to the
table's own dump().

Run extents, seq, windows, flags, the per-sequence array and the totals are compared exactly with
the model after naming unitigs by their normal form, as test_gpu_cdbg.py does for the graph.
Independently of the model, every run's orient(S_U, rev) at pos (mod n_nodes on a circle) must spell
the text, every join must be in the same call's edge list, and the header's properties hold."""
import ctypes
import os
import tempfile

import numpy as np
import pytest

import cdbg_model as cm
import graph_model as m
import kaarme_amd as ka
import key_widths as kw
import path_model as pm
import unitig_model as um
from test_gpu_graph import _bases, _reads, count, make_reads, table_of
from test_gpu_unitig import units_of

pytestmark = pytest.mark.gpu

KC_ERR_ARG, KC_ERR_STATE = -1, -4
RANGES = [(1, 0), (2, 0), (2, 50)]
CDBG_FIELDS = ("unitigs", "circular", "nodes", "bases", "max_nodes", "edges", "dead_ends")
PATH_FIELDS = ("seqs", "windows", "located", "runs", "chains", "threaded")
SEQ_FIELDS = ("first_run", "windows", "located", "runs", "chains", "longest_chain")
SENT32 = 0x5A5A5A5A


# ---- helpers ---------------------------------------------------------------------------------------
def fasta_seqs(data):
    return [l.decode() for l in data.split(b"\n") if l and not l.startswith(b">")]


def run_dicts(runs):
    """a RUN_DTYPE array as the model's dicts; every other flag bit and the reserved word are 0"""
    out = []
    for tp, s, w, u, q, fl, r in runs.tolist():
        assert fl & ~3 == 0 and r == 0 and w >= 1, (tp, s, w, u, q, fl, r)
        out.append({"text_pos": tp, "seq": s, "windows": w, "unitig": u, "pos": q, "rev": fl & ka.RUN_REV,
                    "joined": fl >> 1 & 1})
    return out


def seq_dicts(per):
    assert not per["reserved"].any()
    return [dict(zip(SEQ_FIELDS, row)) for row in zip(*(per[f].tolist() for f in SEQ_FIELDS))]


def check_device_answer(text, k, units, edge_tuples, runs):
    """without the model: every run spells the text, the runs are in text order and disjoint, and the
    header's properties of the joins hold"""
    up = text.upper()
    have = set(edge_tuples)
    for j, r in enumerate(runs):
        s, n, _, circ = units[r["unitig"]]
        assert r["pos"] < n and (circ or r["pos"] + r["windows"] <= n), r
        want = up[r["text_pos"]:r["text_pos"] + r["windows"] + k - 1]
        assert pm.spelled(units[r["unitig"]], k, r["rev"], r["pos"], r["windows"]) == want, r
        if s == m.rc(s):
            assert r["rev"] == 0
        if j:
            b = runs[j - 1]
            assert b["text_pos"] + b["windows"] <= r["text_pos"] and b["seq"] <= r["seq"]
            assert r["joined"] == (b["seq"] == r["seq"] and b["text_pos"] + b["windows"] == r["text_pos"])
        else:
            assert not r["joined"]
        if r["joined"]:
            b = runs[j - 1]
            nb, bcirc = units[b["unitig"]][1], units[b["unitig"]][3]
            assert r["pos"] == 0 and b["pos"] + b["windows"] == nb and not circ and not bcirc, (b, r)
            assert (b["unitig"], b["rev"], r["unitig"], r["rev"]) in have, (b, r)


def check_paths(kc, table, reads, lo=1, hi=0, graph=None):
    """kc.read_paths(reads, lo, hi) == the model on the table; returns the model's answer"""
    k = kc.cfg.k
    text, off = pm.pack(reads)
    want = pm.paths(table, text, off, k, lo, hi, graph=graph)
    units, edges, cst, runs, per, st = want
    cst = cst or dict.fromkeys(CDBG_FIELDS, 0)
    records, bases, got_e, got_cst, got_runs, got_per, got_st = kc.read_paths(reads, lo, hi)
    assert got_cst == cst and got_st == st, (got_cst, cst, got_st, st)
    assert got_runs.shape == (st["runs"],) and got_per.shape == (len(reads),)
    got_units = units_of(records, bases, k, cst["bases"])
    assert um.normalised(got_units) == um.normalised(units)
    tuples = cm.edge_tuples(got_e)
    assert cm.normalised_edges(got_units, tuples) == cm.normalised_edges(units, edges)
    got = run_dicts(got_runs)
    assert all(r["unitig"] < cst["unitigs"] for r in got)
    check_device_answer(text, k, got_units, tuples, got)
    assert pm.normalised_runs(got_units, got) == pm.normalised_runs(units, runs)
    assert seq_dicts(got_per) == per
    assert kc.read_path_stats(reads, lo, hi) == st
    return want


@pytest.fixture(scope="module")
def counted():
    """k -> (counter, its table as a dict, the reads to map), made once; .model(k, lo, hi) -> the
    model's graph, made once"""
    made, models = {}, {}

    def get(k):
        if k not in made:
            data = kw.width_input(k)
            own, other = fasta_seqs(data), fasta_seqs(kw.width_input(k, other=1))
            reads = own[:150] + other[:40] if k <= 65 else own[:30] + other[:8]
            kc = count(data, k)
            made[k] = (kc, table_of(kc), reads)
        return made[k]

    def model(k, lo=1, hi=0):
        if (k, lo, hi) not in models:
            models[k, lo, hi] = cm.cdbg(get(k)[1], lo, hi)
        return models[k, lo, hi]

    get.model = model
    yield get
    for kc, _, _ in made.values():
        kc.close()


# ---- 1. every key width ----------------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", RANGES)
@pytest.mark.parametrize("k", kw.HEAVY_KS)
def test_every_key_width(k, lo, hi, counted):
    kc, table, reads = counted(k)
    _, _, _, runs, per, st = check_paths(kc, table, reads, lo, hi, graph=counted.model(k, lo, hi))
    assert 0 < st["located"] < st["windows"] and st["runs"] > st["chains"] > 0
    assert any(r["joined"] for r in runs) and any(r["rev"] for r in runs) and not all(r["rev"] for r in runs)
    if (lo, hi) == (1, 0):
        assert st["threaded"] > 0


# ---- 2. dense small k ------------------------------------------------------------------------------
@pytest.mark.parametrize("k,n", [(4, 300), (6, 3000)])
def test_dense_small_k(k, n):
    """palindromic nodes, self loops and sides of degree 4: nearly every window is a run of its own"""
    rng = np.random.default_rng(200 + k)
    g = _bases(rng, n)
    with count(b">t\n" + g + b"\n", k, table_slots=1 << 14) as kc:
        table = table_of(kc)
        med = int(np.median(list(table.values())))
        reads = [g.decode(), m.rc(g.decode())[:n // 2], _bases(rng, 200).decode(), "acgtNNacgtacgt" * 3]
        units, _, _, runs, _, _ = check_paths(kc, table, reads)
        assert any(units[r["unitig"]][0] == m.rc(units[r["unitig"]][0]) for r in runs)  # on a palindromic unitig
        check_paths(kc, table, reads, med, 0)
        check_paths(kc, table, reads, 1, med)


# ---- 3. one long chain, 4. a circle ----------------------------------------------------------------
def test_one_long_chain():
    k = 31
    rng = np.random.default_rng(2024)
    read = _bases(rng, 20000)
    with count(b">r\n" + read + b"\n", k, table_slots=1 << 16) as kc:
        s = read.decode()
        _, _, _, runs, per, st = check_paths(kc, table_of(kc), [s, m.rc(s), s[5000:5100].lower()])
        assert [r["windows"] for r in runs] == [20000 - k + 1, 20000 - k + 1, 100 - k + 1] and st["threaded"] == 3


def test_circle_of_500_nodes():
    k = 31
    rng = np.random.default_rng(7)
    circle = _bases(rng, 500)
    with count(_reads(rng, circle * 3, 400, 100), k, table_slots=1 << 14) as kc:
        laps = (circle * 4).decode()[123:123 + 1150 + k - 1]  # 2.3 times round
        units, _, _, runs, per, st = check_paths(kc, table_of(kc), [laps, m.rc(laps)])
        assert [(u[1], u[3]) for u in units] == [(500, True)]
        assert [(r["windows"], r["joined"]) for r in runs] == [(1150, 0), (1150, 0)] and runs[0]["rev"] != runs[1]["rev"]


# ---- 5. several passes -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def passes():
    """a counter with batch_bytes = 32768, its table, and a text of several passes: short reads, one
    sequence longer than a pass, empty and N-only sequences"""
    k = 31
    rng = np.random.default_rng(77)
    genome = _bases(rng, 40000)
    data = _reads(rng, genome, 1500, 100, err=0.005)
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "reads.fasta")
        with open(path, "wb") as f:
            f.write(data)
        kc, _ = ka.count_file(path, k, mode=2, min_abundance=1, table_slots=1 << 18, chunk_size=16384, batch_bytes=32768)
    seqs = fasta_seqs(data)
    reads = seqs[:400] + [genome.decode()] + seqs[400:700] + ["", "N" * 50] + seqs[700:800]
    table = table_of(kc)
    yield kc, table, reads, cm.cdbg(table)
    kc.close()


def test_several_passes(passes):
    kc, table, reads, graph = passes
    text, off = pm.pack(reads)
    assert len(text) > 3 * 32768 and max(len(r) for r in reads) > 32768
    _, _, _, runs, per, st = check_paths(kc, table, reads, graph=graph)
    # the run numbering carries over the pass boundaries
    assert len(reads[400]) > 32768 and per[400]["first_run"] > 0
    assert per[401]["first_run"] == per[400]["first_run"] + per[400]["runs"]
    assert per[-1]["first_run"] + per[-1]["runs"] == st["runs"] and st["runs"] > 600


# ---- 6. the device form ----------------------------------------------------------------------------
def _device_call(kc, text, off, lo, hi, cap_u, cap_b, cap_e, cap_r, guard=16, null=(), shift=0, **kw_):
    """read_paths_device into sentinel-filled buffers of the capacities plus a guard; the host copies.
    null: names of outputs passed as NULL; shift: the text's address is moved off alignment"""
    import torch
    n_seqs = len(off) - 1
    raw = torch.frombuffer(bytearray(b"\n" * shift + text.encode()), dtype=torch.uint8).cuda()
    bufs = {
        "unitigs": torch.full(((cap_u + guard) * 4,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda"),
        "bases": torch.full((cap_b + guard,), 0x5A, dtype=torch.uint8, device="cuda"),
        "edges": torch.full(((cap_e + guard) * 4,), SENT32, dtype=torch.int32, device="cuda"),
        "cdbg_stats": torch.full((8,), -1, dtype=torch.int64, device="cuda"),
        "runs": torch.full(((cap_r + guard) * 8,), SENT32, dtype=torch.int32, device="cuda"),
        "seq": torch.full(((n_seqs + guard) * 8,), SENT32, dtype=torch.int32, device="cuda"),
        "path_stats": torch.full((8 + guard,), -1, dtype=torch.int64, device="cuda"),
    }
    p = {n: (0 if n in null else b.data_ptr()) for n, b in bufs.items()}
    kc.read_paths_device(raw.data_ptr() + shift, len(text), off, lo, hi, p["unitigs"], cap_u, p["bases"], cap_b, p["edges"],
                         cap_e, p["cdbg_stats"], p["runs"], cap_r, p["seq"], p["path_stats"], **kw_)
    torch.cuda.synchronize()
    return {n: b.cpu().numpy() for n, b in bufs.items()}


def _views(h, n_seqs):
    return (h["unitigs"].view(np.uint64), h["bases"], h["edges"].view(np.uint32), h["cdbg_stats"].tolist(),
            h["runs"].view(np.uint32), h["seq"].view(np.uint32), h["path_stats"].tolist())


def _check_device(kc, table, reads, graph, want_host, cap_r=None, null=(), shift=0, **kw_):
    """one device call with full graph capacities and cap_r runs, checked against the model's answer"""
    k = kc.cfg.k
    text, off = pm.pack(reads)
    units, edges, cst, runs, per, st = want_host
    n, nb, ne, nr = cst["unitigs"], cst["bases"], cst["edges"], st["runs"]
    cap_r = nr if cap_r is None else cap_r
    h = _device_call(kc, text, off, 1, 0, n, nb, ne, cap_r, null=null, shift=shift, **kw_)
    hr, hb, he, hcs, hruns, hseq, hps = _views(h, len(reads))
    # nothing behind a capacity, nothing at all into a buffer that was not passed
    assert (hr[n * 4:] == np.uint64(0x5A5A5A5A5A5A5A5A)).all() and (hb[nb:] == 0x5A).all() and (he[ne * 4:] == SENT32).all()
    assert (hruns[cap_r * 8:] == SENT32).all() and (hseq[len(reads) * 8:] == SENT32).all() and hps[8:] == [-1] * 16
    for name in null:
        assert (h[name].view(np.uint8) == h[name].view(np.uint8)[0]).all(), name
    if "cdbg_stats" not in null:
        assert hcs == [cst[f] for f in CDBG_FIELDS] + [0]
    if "path_stats" not in null:
        assert hps[:8] == [st[f] for f in PATH_FIELDS] + [0, 0]  # the totals are always full
    if "seq" not in null:
        assert seq_dicts(hseq[:len(reads) * 8].view(ka.PATH_SEQ_DTYPE)) == per
    if not {"runs", "unitigs", "bases", "edges"} & set(null):
        got_units = units_of(hr[:n * 4], hb, k, nb)
        tuples = cm.edge_tuples(he[:ne * 4].view(ka.EDGE_DTYPE))
        assert cm.normalised_edges(got_units, tuples) == cm.normalised_edges(units, edges)
        got = run_dicts(hruns[:min(cap_r, nr) * 8].view(ka.RUN_DTYPE))
        check_device_answer(text, k, got_units, tuples, got)
        assert pm.normalised_runs(got_units, got) == pm.normalised_runs(units, runs)[:cap_r]
    return h


@pytest.fixture(scope="module")
def small(passes):
    """the passes' counter with a text of one pass, and the model's answer"""
    kc, table, reads, graph = passes
    some = reads[:60] + ["", "acgt"] + reads[700:720]
    text, off = pm.pack(some)
    return kc, table, some, graph, pm.paths(table, text, off, kc.cfg.k, graph=graph)


def test_capacities_bound_the_runs(small):
    kc, table, reads, graph, want = small
    nr = want[5]["runs"]
    assert nr > 20
    for cap_r in (0, 1, nr - 1, nr):
        _check_device(kc, table, reads, graph, want, cap_r=cap_r)


def test_fewer_unitig_records_than_unitigs(small):
    import torch
    kc, table, reads, graph, want = small
    units, edges, cst, runs, per, st = want
    text, off = pm.pack(reads)
    n, nb, ne, nr = cst["unitigs"], cst["bases"], cst["edges"], st["runs"]
    h = _device_call(kc, text, off, 1, 0, n // 2, nb, ne, nr)
    hr, hb, he, hcs, hruns, hseq, hps = _views(h, len(reads))
    assert (hr[(n // 2) * 4:] == np.uint64(0x5A5A5A5A5A5A5A5A)).all()
    got = run_dicts(hruns[:nr * 8].view(ka.RUN_DTYPE))
    assert all(r["unitig"] < n for r in got) and any(r["unitig"] >= n // 2 for r in got)
    assert [(r["text_pos"], r["windows"], r["joined"]) for r in got] == [(r["text_pos"], r["windows"], r["joined"]) for r in runs]
    torch.cuda.synchronize()


@pytest.mark.parametrize("null", [("unitigs",), ("bases",), ("edges",), ("cdbg_stats",), ("runs",), ("seq",),
                                  ("path_stats",), ("unitigs", "bases", "edges", "cdbg_stats", "runs", "seq")])
def test_every_pointer_null_in_turn(null, small):
    kc, table, reads, graph, want = small
    _check_device(kc, table, reads, graph, want, null=null)


def test_side_stream_and_unaligned_text(small, passes):
    import torch
    kc, table, reads, graph, want = small
    before = (kc.finish(), table_of(kc))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _check_device(kc, table, reads, graph, want, stream=s.cuda_stream)
    for shift in (1, 3, 7):
        _check_device(kc, table, reads, graph, want, shift=shift)
    # several passes in the device form, without dev_seq (the context's own per-sequence records)
    big = passes[2]
    text, off = pm.pack(big)
    want_big = pm.paths(table, text, off, kc.cfg.k, graph=graph)
    _check_device(kc, table, big, graph, want_big, null=("seq",))
    # the table is only read: no counter moved, the dump is the same
    assert kc.finish() == before[0] and table_of(kc) == before[1]


# ---- 7. errors and states --------------------------------------------------------------------------
def _host_rc(kc, lo, hi, text, n, off, n_seqs):
    st = ka.kc_path_stats()
    offp = off.ctypes.data if off is not None else None
    return kc.lib.kc_read_paths(kc._ctx, lo, hi, None, None, None, None, text, n, offp, n_seqs, None, None, ctypes.byref(st)), st


def test_argument_and_state_errors(small):
    import torch
    kc, table, reads, graph, want = small
    text, off = ka.pack_sequences(reads[:3])
    n = len(text)
    assert _host_rc(kc, 3, 2, text, n, off, 3)[0] == KC_ERR_ARG  # min_count above max_count
    assert _host_rc(kc, 1, 0, text, n, None, 3)[0] == KC_ERR_ARG  # null offsets
    assert _host_rc(kc, 1, 0, None, n, off, 3)[0] == KC_ERR_ARG  # null text
    assert _host_rc(kc, 1, 0, text, n - 1, off, 3)[0] == KC_ERR_ARG  # offsets pass the end
    bad = off.copy()
    bad[1], bad[2] = off[2], off[1]
    assert _host_rc(kc, 1, 0, text, n, bad, 3)[0] == KC_ERR_ARG  # offsets decrease
    rc, st = _host_rc(kc, 1, 0, text, n, off, 0)
    assert rc == 0 and [getattr(st, f) for f in PATH_FIELDS] == [0] * 6
    rc, st = _host_rc(kc, 1, 0, None, 0, np.zeros(1, dtype=np.uint64), 0)
    assert rc == 0 and st.runs == 0
    with pytest.raises(ka.KcError) as e:
        kc.read_paths(reads[:3], 5, 4)
    assert e.value.code == KC_ERR_ARG and "min_count" in str(e.value)
    buf = torch.zeros(64, dtype=torch.int32, device="cuda")
    dt = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    with pytest.raises(ka.KcError) as e:  # a run is two 16-byte stores
        kc.read_paths_device(dt.data_ptr(), n, off, runs_ptr=buf.data_ptr() + 8, cap_runs=1)
    assert e.value.code == KC_ERR_ARG and "aligned" in str(e.value)
    with pytest.raises(ka.KcError) as e:
        kc.read_paths_device(dt.data_ptr(), n, off, edges_ptr=buf.data_ptr() + 4, cap_edges=1)
    assert e.value.code == KC_ERR_ARG and "aligned" in str(e.value)
    with ka.KmerCounter(ka.Config(k=31, bf_enable=True, est_unique=100000, min_abundance=1)) as nb:
        assert _host_rc(nb, 1, 0, text, n, off, 3)[0] == KC_ERR_STATE
        assert nb.lib.kc_read_paths_device(nb._ctx, 1, 0, None, 0, None, 0, None, 0, None, dt.data_ptr(), n, off.ctypes.data,
                                           3, None, 0, None, None, None) == KC_ERR_STATE
    with count(b">t\nACGTTGCA\n", 1, table_slots=1 << 12) as k1:
        assert _host_rc(k1, 1, 0, text, n, off, 3)[0] == KC_ERR_ARG
    torch.cuda.synchronize()


def test_emptied_table_locates_nothing():
    k = 31
    data = make_reads(k, 300)
    reads = fasta_seqs(data)[:50]
    with count(data, k) as kc:
        table = table_of(kc)
        want = check_paths(kc, table, reads)
        assert want[5]["located"] > 0
        for empty_it in (kc.clear_table, kc.reset):
            empty_it()
            records, bases, edges, cst, runs, per, st = kc.read_paths(reads)
            assert records.shape == (0, 4) and edges.shape == (0,) and runs.shape == (0,)
            assert cst == dict.fromkeys(CDBG_FIELDS, 0)
            assert st == {"seqs": 50, "windows": want[5]["windows"], "located": 0, "runs": 0, "chains": 0, "threaded": 0}
            assert per["windows"].tolist() == [p["windows"] for p in want[4]] and not per["located"].any()
            assert not per["first_run"].any()
            for off, ln, bh in ka.plan_chunks(data, k, ka.FMT_FASTA):
                kc.count_chunk(data[off:off + ln], ka.FMT_FASTA, bool(bh))
            kc.finish()
            assert kc.read_path_stats(reads) == want[5]


# ---- 8. the other calls are not disturbed ----------------------------------------------------------
def test_graph_outputs_equal_unitig_graph_and_nothing_is_disturbed(small):
    kc, table, reads, graph, want = small
    k = kc.cfg.k
    fin = kc.finish()
    before = (kc.unitig_graph(), kc.unitigs(), kc.seq_stats(reads))
    records, bases, edges, cst, _, _, _ = kc.read_paths(reads)
    after = (kc.unitig_graph(), kc.unitigs(), kc.seq_stats(reads))
    assert before[0][3] == after[0][3] == cst and before[1][2] == after[1][2]
    for g in (before[0], after[0]):
        gu, pu = units_of(g[0], g[1], k), units_of(records, bases, k)
        assert um.normalised(gu) == um.normalised(pu)
        assert cm.normalised_edges(gu, cm.edge_tuples(g[2])) == cm.normalised_edges(pu, cm.edge_tuples(edges))
    assert um.normalised(units_of(*before[1][:2], k)) == um.normalised(units_of(*after[1][:2], k))
    assert (before[2] == after[2]).all()
    assert kc.finish() == fin
