"""Counting of packed symbol streams (kc_count_packed_device / kc_bloom_packed_device, the receive
side of the super-k-mer exchange) over hand-built streams, and the window counter that sizes their
buffers (kc_packed_windows_device).

The streams are written with skm_model.pack; what is expected is the oracle's output over the same
sequences as plain lines, and skm_model.packed_windows for the windows.  The `windows` argument of
the two passes is a hint: exact, unknown, eight times too big or too small, or 1, it must give the
same table on every insert path, also for streams whose windows cluster in a few batches (which
wrote past the exact key buffers while the hint's density sized them).  Every case takes a fresh
context, so that a buffer an earlier case grew cannot hide one that is too short."""
import functools

import numpy as np
import pytest

from conftest import oracle_count, text_digest
import kaarme_amd as ka
import skm_model as sm

pytestmark = pytest.mark.gpu

COMP = str.maketrans("ACGT", "TGCA")
SLOTS = 2_000_000
SMALL, LARGE = 64 << 10, 64 << 20  # batch_bytes: several batches, one batch
NAMES = ("sparse_dense", "dense_sparse", "dense_middle", "uniform", "one_run", "no_windows", "polyA", "one_word")
HETEROGENEOUS = ("sparse_dense", "dense_sparse", "dense_middle", "polyA")


def _bases(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes().decode()


def _reads(rng, genome, n, L):
    """n reads of L bases of the genome, every other one reverse-complemented"""
    out = []
    for i, p in enumerate(rng.integers(0, len(genome) - L, n)):
        r = genome[int(p):int(p) + L]
        out.append(r.translate(COMP)[::-1] if i & 1 else r)
    return out


def _sequences(name, k):
    """The streams of the issue: sequences of k bases hold one window per k + 1 symbols, sequences of
    4991 bases nearly one per symbol (4991 + 1 and, for k = 31, 127 and 479, k + 1 are multiples of
    32, so batches can be cut between them).  The reads cover a 60 000-base genome several times,
    so counts differ.  Past k = 51 the sparse part shrinks to keep a stream near 10^6 symbols."""
    rng = np.random.default_rng(1000 + k)
    genome = _bases(rng, 60_000)
    n_sparse = 20_000 if k <= 51 else 640_000 // (k + 1)
    dense = lambda: _reads(rng, genome, 40, 4991)
    sparse = lambda n: _reads(rng, genome, n, k)
    if name == "sparse":
        return sparse(n_sparse)
    if name == "sparse_dense":
        return sparse(n_sparse) + dense()
    if name == "dense_sparse":
        return dense() + sparse(n_sparse)
    if name == "dense_middle":
        return sparse(n_sparse // 2) + dense() + sparse(n_sparse // 2)
    if name == "uniform":
        return _reads(rng, genome, 6000, 150)
    if name == "one_run":
        return [_bases(rng, 300_000)]
    if name == "no_windows":  # runs of 1 .. k - 1 bases between runs of 1 .. 3 breaks and line ends
        lines = []
        for _ in range(1500):
            a, b = rng.integers(1, k, 2)
            lines.append(_bases(rng, int(a)) + "N" * int(rng.integers(1, 4)) + _bases(rng, int(b)))
        return lines
    if name == "polyA":
        return sparse(n_sparse) + dense() + ["A" * 70_000]
    if name == "one_word":
        return [_bases(rng, 31)]
    raise KeyError(name)


class Stream:
    def __init__(self, name, k, tmp):
        import torch
        self.name, self.k = name, k
        seqs = _sequences(name, k)
        self.pk, self.bk = sm.pack(seqs)
        self.n = len(self.pk)
        self.windows = sm.packed_windows(self.bk, k)
        assert self.windows == sum(max(0, len(r) - k + 1) for s in seqs for r in s.split("N"))
        # (2 spare words: the levels may read them)
        self.dpk = torch.from_numpy(np.concatenate([self.pk, np.zeros(2, np.uint64)]).view(np.int64)).cuda()
        self.dbk = torch.from_numpy(np.concatenate([self.bk, np.zeros(2, np.uint32)]).view(np.int32)).cuda()
        self._seqs, self._tmp, self._oracle = seqs, tmp, None

    def oracle(self):
        """(digest, lines) of the oracle's count of the sequences as plain lines, run once"""
        if self._oracle is None:
            src = self._tmp / f"{self.name}_{self.k}.txt"
            out = self._tmp / f"{self.name}_{self.k}.out"
            src.write_text("".join(s + "\n" for s in self._seqs))
            st = oracle_count(str(src), self.k, ["-a", "1"], out)
            assert st["windows"] == self.windows
            lines = open(out).read().splitlines() if out.exists() else []
            self._oracle = (text_digest(str(out)), lines)
        return self._oracle

    def cuts(self, batch, hint):
        return sm.packed_cuts(self.bk, sm.packed_cut_words(batch, self.n, hint))

    def hint(self, kind):
        return {"exact": self.windows, "zero": 0, "x8": 8 * self.windows, "d8": self.windows // 8, "one": 1}[kind]


@pytest.fixture(scope="module")
def stream(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("packed")

    @functools.lru_cache(maxsize=None)  # (a stream is some 100 KB of HBM: all of them stay)
    def get(name, k):
        return Stream(name, k, tmp)

    return get


PATHS = {
    "auto": {},
    "partitioned": {"KC_INSERT_PATH": "partitioned"},
    "exact": {"KC_INSERT_PATH": "exact"},
    "forced": {"KC_INSERT_PATH": "partitioned", "KC_SEG_CAP": "8", "KC_SPILL_CAP": "64"},
}


def _set_path(monkeypatch, path, defer):
    for v in ("KC_INSERT_PATH", "KC_SEG_CAP", "KC_SPILL_CAP", "KC_DEFER"):
        monkeypatch.delenv(v, raising=False)
    for name, v in PATHS[path].items():
        monkeypatch.setenv(name, v)
    if not defer:
        monkeypatch.setenv("KC_DEFER", "0")


def _assert_heterogeneous(s, batch=SMALL):
    """From the model alone: some slice of the cut length holds at least twice the stream's
    average windows per symbol (so a batch sized for the average is at least 2 x too small)."""
    ends = np.concatenate([[0], np.cumsum(sm.window_ends(s.bk, s.k))])
    span = min(32 * sm.packed_cut_words(batch, s.n, s.windows), 32 * s.n)
    densest = int((ends[span:] - ends[:-span]).max())
    assert densest / span >= 2.0 * s.windows / (32 * s.n), (densest, span, s.windows, s.n)


# ---- the window counter ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 31, 32, 33, 51, 127, 479])
def test_window_counter_equals_the_model(k, stream):
    """Whole streams, the sub-ranges that start at each cut of the small batches, and two that start
    inside a run (a range sees only the symbols inside it)."""
    with ka.KmerCounter(ka.Config(k=k, mode=2, min_abundance=1, table_slots=1 << 16)) as kc:
        for name in NAMES:
            s = stream(name, k)
            got = kc.packed_windows_device(s.dpk.data_ptr(), s.dbk.data_ptr(), s.n)
            print(f"{name} k={k}: {s.n} words, {got} windows (model {s.windows})")
            assert got == s.windows, name
            starts = s.cuts(SMALL, s.windows)[1:] + [w for w in (1, 7, s.n - 1) if 0 < w < s.n]
            assert name not in HETEROGENEOUS or len(starts) > 3
            for c in starts:
                got = kc.packed_windows_device(s.dpk.data_ptr() + 8 * c, s.dbk.data_ptr() + 4 * c, s.n - c)
                assert got == sm.packed_windows(s.bk[c:], k), (name, c)
            # a prefix: the range ends with its last word, wherever a run stands
            for c in (1, s.n // 2):
                got = kc.packed_windows_device(s.dpk.data_ptr(), s.dbk.data_ptr(), c)
                assert got == sm.packed_windows(s.bk[:c], k), (name, c)
        assert kc.packed_windows_device(0, 0, 0) == 0


# ---- counting ------------------------------------------------------------------------------------------
def _count_case(stream, monkeypatch, name, k, hint, batch, path, defer):
    s = stream(name, k)
    if name in HETEROGENEOUS:
        _assert_heterogeneous(s)
    _set_path(monkeypatch, path, defer)
    cfg = ka.Config(k=k, mode=2, min_abundance=1, table_slots=SLOTS, batch_bytes=batch)
    with ka.KmerCounter(cfg) as kc:
        kc.count_packed_device(s.dpk.data_ptr(), s.dbk.data_ptr(), s.n, s.hint(hint))
        st = kc.finish()
        dig = kc.output_digest()
    want, _ = s.oracle()
    print(f"{name} k={k} hint={hint} batch={batch} path={path} defer={defer}: windows {st['windows']}, "
          f"fallbacks {st['part_fallbacks']}, deferred {st['deferred_level3']}, lines {dig['lines']}")
    assert st["windows"] == s.windows
    assert ka.same_digest(dig, want), (dig, want)
    nb = len(s.cuts(batch, s.hint(hint)))
    if path == "forced" and s.windows > 64:
        assert st["part_fallbacks"] >= 1
    # the deferred level 3 runs in a pass of several batches through the segmented levels (forced
    # by the path knob; left to itself the cost rule may pick either path for these batches)
    if path in ("partitioned", "forced") and nb >= 2:
        assert (st["deferred_level3"] > 0) == defer
    elif path != "auto" or nb < 2 or not defer:
        assert st["deferred_level3"] == 0


# every stream with an honest hint, in several batches, on the path the cost rule picks
@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("k", [31, 51, 127])
def test_count_with_the_exact_hint(name, k, stream, monkeypatch):
    _count_case(stream, monkeypatch, name, k, "exact", SMALL, "auto", True)


# (stream, k, hint, batch_bytes, path, deferral): wrong hints on every path, with and without the
# deferred level 3, in several batches and in one
CASES = [
    # the stream whose dense part comes last, every wrong hint on every path
    *[("sparse_dense", k, h, SMALL, p, d)
      for k, rows in {31: [("zero", "partitioned", True), ("x8", "exact", True), ("d8", "forced", True),
                           ("one", "auto", True), ("d8", "partitioned", False), ("exact", "partitioned", True)],
                      51: [("zero", "forced", True), ("x8", "partitioned", True), ("d8", "exact", True),
                           ("one", "partitioned", False), ("d8", "auto", True), ("exact", "forced", False)],
                      127: [("zero", "exact", True), ("x8", "forced", False), ("d8", "partitioned", True),
                            ("one", "forced", True), ("exact", "partitioned", False), ("zero", "auto", True)],
                      479: [("exact", "auto", True), ("d8", "partitioned", True), ("one", "forced", True),
                            ("x8", "exact", True)]}.items()
      for h, p, d in rows],
    # the dense part first, and between two sparse parts
    *[("dense_sparse", 51, "d8", SMALL, p, True) for p in PATHS],
    ("dense_sparse", 31, "exact", SMALL, "partitioned", True),
    ("dense_sparse", 127, "zero", SMALL, "forced", True),
    ("dense_middle", 31, "zero", SMALL, "partitioned", True),
    ("dense_middle", 31, "d8", SMALL, "forced", True),
    ("dense_middle", 51, "exact", SMALL, "partitioned", False),
    ("dense_middle", 127, "d8", SMALL, "exact", True),
    # heavy records (a 70 000-base poly-A run) in a packed, deferred pass
    *[("polyA", k, h, SMALL, p, d) for k in (31, 51)
      for h, p, d in (("exact", "partitioned", True), ("exact", "partitioned", False), ("x8", "forced", True),
                      ("d8", "exact", True))],
    ("polyA", 127, "exact", SMALL, "partitioned", True),
    # one batch far above the cut length (no cut exists), streams without windows, one word
    *[("one_run", k, h, SMALL, p, True) for k, h, p in ((31, "one", "partitioned"), (51, "d8", "exact"),
                                                         (127, "x8", "forced"), (31, "zero", "forced"))],
    ("no_windows", 31, "zero", SMALL, "partitioned", True),
    ("no_windows", 51, "x8", SMALL, "exact", True),
    ("one_word", 31, "zero", SMALL, "partitioned", True),
    ("one_word", 31, "exact", LARGE, "forced", True),
    ("uniform", 31, "d8", SMALL, "partitioned", True),
    ("uniform", 51, "one", SMALL, "forced", True),
    ("uniform", 127, "zero", SMALL, "exact", True),
    # one batch for the whole stream
    *[("sparse_dense", k, h, LARGE, p, True) for k, h, p in ((31, "exact", "auto"), (31, "d8", "exact"),
                                                              (51, "d8", "partitioned"), (51, "one", "forced"),
                                                              (127, "zero", "partitioned"), (127, "d8", "exact"))],
    ("uniform", 51, "exact", LARGE, "partitioned", True),
    ("polyA", 31, "zero", LARGE, "partitioned", True),
]


@pytest.mark.parametrize("name,k,hint,batch,path,defer", sorted(CASES, key=lambda c: (c[0], c[1])),
                         ids=lambda v: str(v))
def test_count_does_not_depend_on_hint_or_path(name, k, hint, batch, path, defer, stream, monkeypatch):
    _count_case(stream, monkeypatch, name, k, hint, batch, path, defer)


def test_second_pass_regrows_the_buffers(stream, monkeypatch):
    """One context: a sparse stream (one window per 32 symbols), kc_reset, then a stream of one
    window per symbol with a hint far too small, each in one batch on the exact layout: the key
    buffers the first pass left are too short for the second."""
    _set_path(monkeypatch, "exact", True)
    k = 31
    a, b = stream("sparse", k), stream("one_run", k)
    assert b.windows > 8 * a.windows
    cfg = ka.Config(k=k, mode=2, min_abundance=1, table_slots=SLOTS, batch_bytes=LARGE)
    with ka.KmerCounter(cfg) as kc:
        for s, hint in ((a, a.windows), (b, a.windows // 8)):
            kc.reset()
            kc.count_packed_device(s.dpk.data_ptr(), s.dbk.data_ptr(), s.n, hint)
            st = kc.finish()
            assert st["windows"] == s.windows
            assert ka.same_digest(kc.output_digest(), s.oracle()[0]), s.name


# ---- the Bloom job of an owner ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sparse_dense", "uniform"])
@pytest.mark.parametrize("hint", ["exact", "zero", "d8"])
@pytest.mark.parametrize("path", ["partitioned", "forced"])
def test_bloom_job_over_a_packed_stream(name, hint, path, stream, monkeypatch):
    """kc_bloom_packed_device, kc_bloom_finalize, kc_count_packed_device: the k-mers seen twice or
    more are the oracle's exactly, and a count-1 line is a true singleton."""
    k = 51
    s = stream(name, k)
    if name in HETEROGENEOUS:
        _assert_heterogeneous(s)
    _set_path(monkeypatch, path, True)
    cfg = ka.Config(k=k, mode=2, min_abundance=1, bf_enable=True, est_unique=1_000_000, batch_bytes=SMALL)
    with ka.KmerCounter(cfg) as kc:
        kc.bloom_packed_device(s.dpk.data_ptr(), s.dbk.data_ptr(), s.n, s.hint(hint))
        kc.bloom_finalize()
        kc.count_packed_device(s.dpk.data_ptr(), s.dbk.data_ptr(), s.n, s.hint(hint))
        st = kc.finish()
        lines = kc.lines()
    if path == "forced":
        assert st["part_fallbacks"] >= 1
    exact = dict(l.split() for l in s.oracle()[1])
    assert sorted(l for l in lines if int(l.split()[1]) >= 2) == sorted(f"{a} {c}" for a, c in exact.items()
                                                                        if int(c) >= 2)
    assert all(exact.get(l.split()[0]) == "1" for l in lines if l.endswith(" 1"))
