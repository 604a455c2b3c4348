"""GPU: queries of the counted full-key table -- kc_lookup / kc_lookup_device (the count of given
k-mers) and kc_histogram (the abundance spectrum).

Expected values come from the C oracle (``-a 1``) or from kc_dump, which the parity tests pin to
the oracle; never from the query path itself.  Inputs are kc_gen reads of 3000 x max(150, k + 100)
bp over a 40 kbp genome with 0.2 % errors (as test_gpu_compact.py), or small golden inputs.
"""
import subprocess

import numpy as np
import pytest

from conftest import GEN, load_cases, oracle_count
import kaarme_amd as ka

pytestmark = pytest.mark.gpu

# W = 1, 1, 2, 2, 2, 3, 4, 5, 7, 8, 15; slots per bucket 8, 5, 4, 3, 2, 1; k % 32 == 0 three times
KS = [5, 31, 32, 33, 63, 64, 127, 128, 200, 255, 479]
KC_ERR_ARG, KC_ERR_STATE = -1, -4


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """k -> path of the generated reads (made once per module)."""
    work = tmp_path_factory.mktemp("query_reads")
    cache = {}

    def get(k):
        L = max(150, k + 100)
        if L not in cache:
            fa = work / f"r{L}.fasta"
            subprocess.run([GEN, str(fa), "3000", str(L), "40000", "-e", "0.002"], check=True)
            cache[L] = str(fa)
        return cache[L]

    return get


@pytest.fixture(scope="module")
def oracle_lines(tmp_path_factory, reads):
    """(k, mode) -> (k-mer strings, counts) of the oracle's -a 1 output (run once per module)."""
    work = tmp_path_factory.mktemp("query_oracle")
    cache = {}

    def get(k, mode=2, path=None):
        key = (k, mode, path)
        if key not in cache:
            out = work / f"o{len(cache)}.txt"
            oracle_count(path or reads(k), k, ["-m", str(mode), "-a", "1"], out)
            kmers, counts = [], []
            with open(out) as f:
                for line in f:
                    s, c = line.split()
                    kmers.append(s)
                    counts.append(int(c))
            cache[key] = (kmers, np.array(counts, dtype=np.uint32))
        return cache[key]

    return get


def _codes(keys, k):
    W = keys.shape[1]
    codes = np.empty((keys.shape[0], k), dtype=np.uint8)
    for j in range(k):
        bit = 2 * (k - 1 - j)
        codes[:, j] = (keys[:, W - 1 - bit // 64] >> np.uint64(bit % 64)) & np.uint64(3)
    return codes


def _pack(codes, k):
    W = ka.words_for_k(k)
    keys = np.zeros((codes.shape[0], W), dtype=np.uint64)
    for j in range(k):
        bit = 2 * (k - 1 - j)
        keys[:, W - 1 - bit // 64] |= codes[:, j].astype(np.uint64) << np.uint64(bit % 64)
    return keys


def _revcomp_keys(keys, k):
    return _pack((3 - _codes(keys, k))[:, ::-1], k)


def _as_dict(full):
    return {tuple(r[:-1]): int(r[-1]) for r in full.tolist()}


def _absent(full, k, n, seed):
    """n random k-mers, canonical or not (expected counts come from the dump's dictionary)."""
    rng = np.random.default_rng(seed)
    return _pack(rng.integers(0, 4, size=(n, k), dtype=np.uint8), k)


def _canonical_expect(d, keys, k):
    """Expected counts of keys of either strand: the dump holds canonical keys."""
    rc = _revcomp_keys(keys, k)
    return np.array([d.get(tuple(a), 0) or d.get(tuple(b), 0) for a, b in zip(keys.tolist(), rc.tolist())],
                    dtype=np.uint32)


# ---- 1. every key width and slot count ---------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_lookup_every_key_width(k, reads):
    kc, st = ka.count_file(reads(k), k, mode=2, min_abundance=1, table_slots=1 << 20)
    with kc:
        full = kc.dump()
        assert len(full) == st["distinct"] > 0
        keys, counts = np.ascontiguousarray(full[:, :-1]), full[:, -1].astype(np.uint32)
        d = _as_dict(full)
        got = kc.lookup(keys)
        assert got.dtype == np.uint32
        assert (got == counts).all()
        assert (kc.lookup(_revcomp_keys(keys, k)) == counts).all()
        flipped = keys[:200].copy()
        flipped[:, -1] ^= np.uint64(1)  # the last character's low bit
        assert (kc.lookup(flipped) == _canonical_expect(d, flipped, k)).all()
        # a bit at position 2k: not a k-mer
        W = keys.shape[1]
        bad = keys[:50].copy()
        bad[:, W - 1 - (2 * k) // 64] |= np.uint64(1) << np.uint64((2 * k) % 64)
        assert not kc.lookup(bad).any()


@pytest.mark.parametrize("k", [31, 51])
def test_lookup_oracle_lines(k, reads, oracle_lines):
    """Every line of the oracle's -a 1 output looks up to its count (k = 51: two-word keys)."""
    kc, st = ka.count_file(reads(k), k, mode=2, min_abundance=1, table_slots=1 << 20)
    with kc:
        kmers, want = oracle_lines(k)
        assert len(kmers) == st["distinct"]
        assert (kc.lookup(ka.encode_kmers(kmers, k)) == want).all()
        assert (kc.lookup(ka.encode_kmers([s.lower() for s in kmers[:500]], k)) == want[:500]).all()


# ---- 2. group and wave tails --------------------------------------------------------------------
@pytest.mark.parametrize("k", [31, 51])
def test_lookup_tails_and_sentinels(k, reads):
    import torch
    SENT = 0x5EA7BEEF
    kc, _ = ka.count_file(reads(k), k, mode=2, min_abundance=1, table_slots=1 << 20)
    with kc:
        full = kc.dump()
        rng = np.random.default_rng(3)
        pick = full[rng.permutation(len(full))[:600]]
        mixed = np.concatenate([pick[:, :-1], _absent(full, k, 400, 4)])
        want = _canonical_expect(_as_dict(full), mixed, k)
        assert want[:600].all() and (want == 0).sum() >= 390
        order = rng.permutation(len(mixed))
        mixed, want = np.ascontiguousarray(mixed[order]), want[order]
        for n in (0, 1, 15, 17, 63, 65, 257, 1000):
            dk = torch.from_numpy(mixed[:max(n, 1)].view(np.int64)).cuda()
            out = torch.full((n + 32,), SENT, dtype=torch.int32, device="cuda")
            kc.lookup_device(dk.data_ptr(), n, out.data_ptr() + 16 * 4)
            torch.cuda.synchronize()
            res = out.cpu().numpy()
            assert (res[:16] == SENT).all() and (res[16 + n:] == SENT).all(), n
            assert (res[16:16 + n].view(np.uint32) == want[:n]).all(), n
        assert len(kc.lookup(np.zeros((0, full.shape[1] - 1), dtype=np.uint64))) == 0


# ---- 3. long probe runs and the wrap inside a region -------------------------------------------
@pytest.mark.parametrize("k", [31, 51])
def test_lookup_in_a_full_table(k, reads):
    """table_slots = the distinct count: the table is as small as the engine makes it for this input
    (25 % headroom), so probe sequences run over several buckets and wrap inside regions."""
    kc0, st0 = ka.count_file(reads(k), k, mode=2, min_abundance=1, table_slots=1 << 20)
    kc0.close()
    kc, st = ka.count_file(reads(k), k, mode=2, min_abundance=1, table_slots=st0["distinct"])
    with kc:
        assert st["distinct"] == st0["distinct"]
        # (the engine rounds the region count up to its partition fan-outs: load 0.74 at k = 31 and
        # 0.66 at k = 51 here, against 0.03 - 0.07 in the 2^20-slot tables of the other tests)
        assert st["table_slots"] < 2 * st["distinct"]
        full = kc.dump()
        keys = np.ascontiguousarray(full[:, :-1])
        assert (kc.lookup(keys) == full[:, -1].astype(np.uint32)).all()
        absent = _absent(full, k, 5000, 9)
        assert (kc.lookup(absent) == _canonical_expect(_as_dict(full), absent, k)).all()
        near = keys[:5000].copy()
        near[:, -1] ^= np.uint64(2)
        assert (kc.lookup(near) == _canonical_expect(_as_dict(full), near, k)).all()


# ---- 4. saturation and wrap of counts -----------------------------------------------------------
@pytest.mark.parametrize("mode,want", [(2, 16383), (0, (20000 - 30) % 65536)])
def test_lookup_saturated_and_wrapped_counts(mode, want, tmp_path):
    fa = tmp_path / "polya.fasta"
    fa.write_text(">a\n" + "A" * 20000 + "\n>b\n" + "ACGT" * 50 + "\n")
    k = 31
    kc, st = ka.count_file(str(fa), k, mode=mode, min_abundance=1, table_slots=1 << 16)
    with kc:
        got = kc.lookup(ka.encode_kmers(["A" * k, "T" * k, "a" * k], k))
        assert got.tolist() == [want, want, want]
        h = kc.histogram(16384)
        assert h.sum() == st["distinct"]
        if mode == 2:
            assert h[16383] == 1  # the saturated k-mer
        else:
            assert h[16383] == 1 and kc.histogram(65537)[want] == 1


# ---- 5. table keys ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [31, 51])
def test_lookup_table_keys_of_routed_windows(k, reads):
    import torch
    with open(reads(k), "rb") as f:
        data = f.read()
    img = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    chunks = ka.plan_chunks(data, k, ka.FMT_FASTA)
    batch = len(data) + 4096 * (len(chunks) + 1)
    W = ka.words_for_k(k)
    cap = sum((ln + 4095) // 4096 * 4096 for _, ln, _ in chunks) + len(chunks)  # keys: staged bytes + chunks
    cfg = dict(k=k, mode=2, min_abundance=1, table_slots=1 << 20, batch_bytes=batch)
    with ka.KmerCounter(ka.Config(**cfg)) as kc, ka.KmerCounter(ka.Config(**cfg)) as router:
        kc.count_device(img.data_ptr(), chunks, ka.FMT_FASTA)
        st = kc.finish()
        counts = kc.dump()[:, -1].astype(np.int64)
        per_v = np.bincount(counts, minlength=16384)
        for nshards in (1, 3):
            buf = torch.zeros(cap * W, dtype=torch.int64, device="cuda")
            groups = router.route_device(img.data_ptr(), chunks, ka.FMT_FASTA, nshards, buf.data_ptr(), cap)
            n = sum(groups)
            assert n == st["windows"]
            out = torch.zeros(n, dtype=torch.int32, device="cuda")
            kc.lookup_device(buf.data_ptr(), n, out.data_ptr(), table_keys=True)
            torch.cuda.synchronize()
            res = out.cpu().numpy().astype(np.int64)
            assert (res > 0).all()
            got = np.bincount(res, minlength=16384)
            v = np.arange(16383)
            assert (got[:16383] == v * per_v[:16383]).all()
        # a table key with word 0 == 0 is no key
        z = np.zeros((3, W), dtype=np.uint64)
        z[:, 1:] = 5
        assert not kc.lookup(z, table_keys=True).any()


def test_lookup_bad_layout_and_null_arrays(reads):
    kc, _ = ka.count_file(reads(31), 31, mode=2, min_abundance=1, table_slots=1 << 20)
    with kc:
        out = np.zeros(4, dtype=np.uint32)
        keys = np.zeros((4, 1), dtype=np.uint64)
        assert kc.lib.kc_lookup(kc._ctx, keys.ctypes.data, 4, 2, out.ctypes.data) == KC_ERR_ARG
        assert kc.lib.kc_lookup(kc._ctx, None, 4, 0, out.ctypes.data) == KC_ERR_ARG
        assert kc.lib.kc_lookup(kc._ctx, keys.ctypes.data, 4, 0, None) == KC_ERR_ARG
        assert kc.lib.kc_lookup(kc._ctx, None, 0, 0, None) == 0
        assert kc.lib.kc_lookup_device(kc._ctx, None, 0, 1, None, None) == 0
        assert kc.lib.kc_lookup_device(kc._ctx, None, 1, 0, None, None) == KC_ERR_ARG


# ---- 6. state -----------------------------------------------------------------------------------
def test_queries_after_clear_and_reset(reads):
    k = 31
    kc, st = ka.count_file(reads(k), k, mode=2, min_abundance=1, table_slots=1 << 20)
    with kc:
        full = kc.dump()
        keys = np.ascontiguousarray(full[:, :-1])
        before = kc.finish()
        assert (kc.lookup(keys) == full[:, -1].astype(np.uint32)).all()
        assert kc.histogram().sum() == st["distinct"]
        assert kc.finish() == before == st  # the queries change no counter
        kc.clear_table()
        assert not kc.lookup(keys).any()
        assert not kc.histogram().any()
        kc.reset()
        assert not kc.lookup(keys).any()
        assert not kc.histogram().any()


def test_queries_need_a_table():
    with ka.KmerCounter(ka.Config(k=31, bf_enable=True, est_unique=100000, min_abundance=1)) as kc:
        with pytest.raises(ka.KcError) as e:
            kc.lookup(np.zeros((1, 1), dtype=np.uint64))
        assert e.value.code == KC_ERR_STATE
        with pytest.raises(ka.KcError) as e:
            kc.histogram()
        assert e.value.code == KC_ERR_STATE


BLOOM_CASES = [c for c in load_cases()["cases"]
               if c["input"] == "reads_w60.fasta" and "-b" in c["args"] and c["args"][-2:] == ["-a", "1"]]


@pytest.mark.parametrize("case", BLOOM_CASES, ids=lambda c: f"k{c['k']}")
def test_lookup_after_a_bloom_job(case, golden_input):
    a = case["args"]
    mode = int(a[a.index("-m") + 1]) if "-m" in a else 2
    k = case["k"]
    kc, st = ka.count_file(golden_input(case["input"]), k, mode=mode, min_abundance=1, bf_enable=True,
                           est_unique=int(a[a.index("-u") + 1]))
    with kc:
        full = kc.dump()
        assert len(full) == st["distinct"] > 0
        keys = np.ascontiguousarray(full[:, :-1])
        assert (kc.lookup(keys) == full[:, -1].astype(np.uint32)).all()
        absent = _absent(full, k, 1000, 1)
        assert (kc.lookup(absent) == _canonical_expect(_as_dict(full), absent, k)).all()
        assert kc.histogram().sum() == len(full)


@pytest.mark.parametrize("k", [31, 51])
def test_lookup_after_deferred_level3(k, monkeypatch):
    """A device image counted in five staging batches through the partitioned levels (the deferred
    level 3 inserts them in groups): lookup equals dump."""
    import torch
    monkeypatch.setenv("KC_INSERT_PATH", "partitioned")
    lib = ka.load_library()
    n, L = 12_000, 150
    nbytes = lib.kc_synth_bytes(0, n, L, 0)
    img = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    assert lib.kc_synth_device(img.data_ptr(), 0, n, 5, 400_000, L, 0, 0.01, 0.001, 0) == 0
    torch.cuda.synchronize()
    host = bytes(img.cpu().numpy())
    chunks = ka.plan_chunks(host, k, ka.FMT_FASTA, 200_000)
    with ka.KmerCounter(ka.Config(k=k, mode=2, min_abundance=1, table_slots=4_000_000, batch_bytes=400 << 10)) as kc:
        kc.count_device(img.data_ptr(), chunks, ka.FMT_FASTA)
        st = kc.finish()
        assert st["deferred_level3"] >= 1 and len(host) > 3 * (400 << 10)
        full = kc.dump()
        assert len(full) == st["distinct"]
        assert (kc.lookup(np.ascontiguousarray(full[:, :-1])) == full[:, -1].astype(np.uint32)).all()
        assert kc.histogram().sum() == st["distinct"]
        assert kc.finish() == st


# ---- 7. histogram -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [2, 0])
@pytest.mark.parametrize("k", KS)
def test_histogram(k, mode, reads, oracle_lines):
    kc, st = ka.count_file(reads(k), k, mode=mode, min_abundance=1, table_slots=1 << 20)
    with kc:
        # the oracle's counts up to two-word keys; the dump (pinned to the oracle by the parity and
        # compact tests) for wider keys
        counts = oracle_lines(k, mode)[1] if k <= 64 else kc.dump()[:, -1]
        counts = counts.astype(np.int64)
        assert len(counts) == st["distinct"]
        h = kc.histogram(16385)
        assert h.dtype == np.uint64 and h.shape == (16385,)
        assert (h == np.bincount(np.minimum(counts, 16384), minlength=16385)).all()
        assert h.sum() == st["distinct"]
        assert (kc.histogram(4) == np.bincount(np.minimum(counts, 3), minlength=4)).all()
        assert (kc.histogram() == h).all()
        for bad in (1, 65538, 0):
            with pytest.raises(ka.KcError) as e:
                kc.histogram(bad)
            assert e.value.code == KC_ERR_ARG


# ---- 8. asynchrony ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [31, 51])
def test_lookup_device_on_a_side_stream(k, reads):
    import torch
    kc, _ = ka.count_file(reads(k), k, mode=2, min_abundance=1, table_slots=1 << 20)
    with kc:
        full = kc.dump()
        keys = np.ascontiguousarray(np.concatenate([full[:, :-1], _absent(full, k, 3000, 2)]))
        want = kc.lookup(keys)
        assert (want[:len(full)] == full[:, -1].astype(np.uint32)).all()
        src = torch.from_numpy(keys.view(np.int64)).pin_memory()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            dk = torch.empty(src.shape, dtype=torch.int64, device="cuda")
            dk.copy_(src, non_blocking=True)
            out = torch.full((len(keys),), -1, dtype=torch.int32, device="cuda")
            kc.lookup_device(dk.data_ptr(), len(keys), out.data_ptr(), stream=s.cuda_stream)
        torch.cuda.synchronize()
        assert (out.cpu().numpy().view(np.uint32) == want).all()
