"""GPU: a context's whole life, over and over, and the profiling brackets.

A context owns its device and pinned memory and every call frees its own temporaries, so
creating, using and closing contexts in a loop must leave the free HBM where it was; and the
event quadruples of the profiling brackets must come back to the pool, so the same sequence
timed twice reports the same launches.
"""
import hashlib

import numpy as np
import pytest

import kaarme_amd as ka

pytestmark = pytest.mark.gpu

CYCLES = 10
# Free HBM after the last cycle against after cycle 2 (the first cycles warm the runtime's own
# pools).  The same loop at the parent commit, whose kc_destroy freed every buffer by hand, read
# a drift of DRIFT_PARENT = 0 bytes at k = 31 and at k = 51 on an MI355X (and 0 with the owners);
# one allocation granule of the runtime (2 MiB) on top is the bound.  One leaked context is many
# times this: its table alone takes 20 MiB or more.
DRIFT_PARENT = 0
GRANULE = 2 << 20
BOUND = DRIFT_PARENT + GRANULE


def _rows(d):
    return d[np.lexsort(d.T[::-1])]


def _cycle(path, k, out):
    """One life of a context; everything it computed, in an order-free form."""
    kc, st = ka.count_file(path, k, mode=2, table_slots=1 << 20)
    with kc:
        full = kc.dump()
        order = np.lexsort(full[:, :-1].T[::-1])
        keys = np.ascontiguousarray(full[order, :-1])
        res = {"stats": (st["windows"], st["distinct"]), "dump": full[order]}
        res["lookup"] = kc.lookup(keys)
        res["hist"] = kc.histogram()
        kc.write(out)
        with open(out, "rb") as f:
            res["text"] = hashlib.sha256(b"".join(sorted(f.read().splitlines(keepends=True)))).hexdigest()
        res["digest"] = kc.output_digest()
        info = kc.compact()
        res["compact"] = (info["slots"], info["kmers"], info["chain_starts"])
        res["compact_lookup"] = kc.compact_lookup(keys)
        res["compact_dump"] = _rows(kc.compact_dump()[0])
    return res


@pytest.mark.parametrize("k", [31, 51])
def test_contexts_give_their_memory_back(k, golden_input, tmp_path):
    import torch
    path = golden_input("reads.txt")
    out = str(tmp_path / "out.txt")
    torch.cuda.init()
    first = last = None
    free2 = None
    for i in range(CYCLES):  # (no torch tensor is created in here)
        last = _cycle(path, k, out)
        if i == 0:
            first = last
        if i == 1:
            free2 = torch.cuda.mem_get_info()[0]
    drift = free2 - torch.cuda.mem_get_info()[0]
    print(f"k={k}: free HBM fell by {drift} bytes from cycle 2 to cycle {CYCLES}")
    assert len(first["dump"]) > 1000 and first["lookup"].all()
    for name in first:
        a, b = first[name], last[name]
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b, name
    assert drift <= BOUND, f"free HBM fell by {drift} bytes over {CYCLES - 2} context lives"


def test_profiling_brackets_and_event_pool(golden_input):
    """kc_get_timing: a single-batch device image is one full quadruple (launches == 1), an insert
    of received keys a {-, -, start, end} bracket (launches == 0, count_ms > 0); the same sequence
    again reports the same, so no event is lost from the pool or used twice."""
    import torch
    k = 31
    path = golden_input("reads.txt")
    with open(path, "rb") as f:
        data = f.read()
    fmt = ka.detect_format(path, data[0])
    chunks = ka.plan_chunks(data, k, fmt)
    img = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cfg = ka.Config(k=k, mode=2, min_abundance=1, table_slots=1 << 20, batch_bytes=len(data) + 4096 * (len(chunks) + 1))
    cap = sum((ln + 4095) // 4096 * 4096 for _, ln, _ in chunks) + len(chunks)
    keys = torch.zeros(cap, dtype=torch.int64, device="cuda")
    with ka.KmerCounter(cfg) as router:
        n = sum(router.route_device(img.data_ptr(), chunks, fmt, 1, keys.data_ptr(), cap))
    n_keys = min(n, 4000)
    assert n_keys > 1000

    with ka.KmerCounter(cfg) as kc:
        def sequence():
            kc.profile(True)
            kc.timing()  # (drops what is pending)
            kc.count_device(img.data_ptr(), chunks, fmt)
            t1 = kc.timing()
            assert t1["launches"] == 1 and t1["tokenize_ms"] > 0 and t1["count_ms"] > 0, t1
            kc.insert_keys_device(keys.data_ptr(), n_keys)
            t2 = kc.timing()
            assert t2["launches"] == 0 and t2["count_ms"] > 0, t2
            return t1["launches"], t2["launches"]

        assert sequence() == sequence()
