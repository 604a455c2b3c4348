"""Pure-Python model of the sequence queries (kc_text_counts*, kc_seq_stats*): slides over the text,
breaks on every non-ACGT byte, makes each window canonical by string reverse complement and looks
it up in a {canonical k-mer: T(c)} dictionary (the C oracle's ``-a 1`` output).  Independent of
the code under test."""
import re

NO_KMER = 0xFFFFFFFF
_COMP = bytes.maketrans(b"ACGT", b"TGCA")
_RUN = re.compile(rb"[ACGTacgt]+")
FIELDS = ("windows", "present", "solid", "min", "median", "max", "sum")


def revcomp(s: bytes) -> bytes:
    return s.translate(_COMP)[::-1]


def canonical(s: bytes) -> bytes:
    """The smaller of an upper-case k-mer and its reverse complement (A < C < G < T)."""
    r = revcomp(s)
    return s if s <= r else r


def oracle_dict(path) -> dict:
    """The oracle's "<KMER> <count>" lines as {canonical k-mer bytes: count}."""
    d = {}
    with open(path, "rb") as f:
        for line in f:
            s, c = line.split()
            d[canonical(s)] = int(c)
    return d


def text_counts(text: bytes, k: int, d: dict, lo: int = 0, hi: int = None) -> list:
    """counts[p - lo] for p in [lo, hi): d's count (0 if absent) of the canonical k-mer of
    text[p : p + k] when all its bytes are bases and p + k <= hi, else NO_KMER."""
    hi = len(text) if hi is None else hi
    out = [NO_KMER] * (hi - lo)
    get = d.get
    for m in _RUN.finditer(text[lo:hi]):  # maximal runs of bases: a window lies inside one
        n = m.end() - m.start()
        if n < k:
            continue
        fwd = m.group().upper()
        rc = revcomp(fwd)  # the window fwd[p : p + k] is rc[n - p - k : n - p] on the other strand
        a = m.start()
        for p in range(n - k + 1):
            f, r = fwd[p:p + k], rc[n - p - k:n - p]
            out[a + p] = get(f if f <= r else r, 0)
    return out


def stats_of(values, solid_min: int) -> dict:
    """kc_seq_stat of the counts of one sequence's windows (NO_KMER entries are no windows)."""
    v = sorted(x for x in values if x != NO_KMER)
    if not v:
        return dict.fromkeys(FIELDS, 0)
    return {"windows": len(v), "present": sum(x >= 1 for x in v), "solid": sum(x >= solid_min for x in v),
            "min": v[0], "median": v[(len(v) - 1) // 2], "max": v[-1], "sum": sum(v)}


def seq_stats(text: bytes, offsets, k: int, d: dict, solid_min: int = 1) -> list:
    """One stats dict per sequence [offsets[i], offsets[i + 1]): its windows lie inside it."""
    off = [int(o) for o in offsets]
    return [stats_of(text_counts(text, k, d, off[i], off[i + 1]), solid_min) for i in range(len(off) - 1)]
