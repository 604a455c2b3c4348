"""CPU: the pure-Python model of the read correction (correct_model.py) on hand cases, and against a
brute-force evaluation of the rule that shares nothing with it but the dictionary."""
import random

import correct_model
from correct_model import FIELDS, correct, guarantee_violations
from seq_model import canonical

K7 = b"ACGGTCA"


def _table(*kmers, count=5):
    return {canonical(s): count for s in kmers}


def _row(st):
    return tuple(st[f] for f in FIELDS)


def test_hand_cases_of_a_read_of_k_bases():
    """k = 7, the read ACGGTCA: its one window covers every position, so all seven are candidates."""
    # one alternative works at position 0
    out, (st,) = correct(K7, [0, 7], 7, _table(b"TCGGTCA"), 2)
    assert out == b"TCGGTCA" and _row(st) == (7, 1, 0, 0)
    # two alternatives work at position 0
    out, (st,) = correct(K7, [0, 7], 7, _table(b"TCGGTCA", b"CCGGTCA"), 2)
    assert out == K7 and _row(st) == (7, 0, 1, 0)
    # positions 0 and 6 are both accepted, closer than k: both dropped
    out, (st,) = correct(K7, [0, 7], 7, _table(b"TCGGTCA", b"ACGGTCT"), 2)
    assert out == K7 and _row(st) == (7, 0, 0, 2)
    # a count below the threshold does not make an alternative work; nothing in the table at all
    assert correct(K7, [0, 7], 7, _table(b"TCGGTCA", count=1), 2) == (K7, [dict(zip(FIELDS, (7, 0, 0, 0)))])
    assert correct(K7, [0, 7], 7, {}, 0) == (K7, [dict(zip(FIELDS, (7, 0, 0, 0)))])
    # the read itself is solid: no candidate; a shorter read: no window
    assert _row(correct(K7, [0, 7], 7, _table(K7), 2)[1][0]) == (0, 0, 0, 0)
    assert _row(correct(K7[:6], [0, 6], 7, _table(K7), 2)[1][0]) == (0, 0, 0, 0)


CLEAN45 = b"ACGTTGCAAGGCTTAACCGGATATCGCGTAGCTAGGATCCTTGAC"


def _clean_table(seq, k, count=3):
    return {canonical(seq[p:p + k]): count for p in range(len(seq) - k + 1)}


def test_lower_case_error_and_an_n():
    """One lower-case wrong base and an N ten bases later: the windows over the N do not exist, the
    others over the error are weak; one candidate, one correction, the letter case kept."""
    k = 7
    # no 7-mer repeats on its strand (AGGATCC and GGATCCT are one canonical k-mer)
    assert len(CLEAN45) == 45 and len(_clean_table(CLEAN45, k)) == 38
    bad = bytearray(CLEAN45)
    assert CLEAN45[20:21] == b"A"
    bad[20] = ord("g")
    bad[30] = ord("N")
    bad = bytes(bad)
    out, (st,) = correct(bad, [0, 45], k, _clean_table(CLEAN45, k), 2)
    want = bytearray(bad)
    want[20] = ord("a")
    assert out == bytes(want) and _row(st) == (1, 1, 0, 0)
    assert guarantee_violations(bad, out, [0, 45], k, _clean_table(CLEAN45, k), 2) == []


def test_error_next_to_a_joint_without_a_break_byte():
    """Two sequences adjacent with no break byte: no window spans the joint, so an error within k - 1
    of it is covered only by the windows of its own sequence."""
    k = 7
    d = _clean_table(CLEAN45, k)
    bad = bytearray(CLEAN45)
    bad[22] = ord("C")  # clean: T; sequence 0 is [0, 25), sequence 1 [25, 45)
    bad[26] = ord("A")  # clean: G
    bad = bytes(bad)
    out, st = correct(bad, [0, 25, 45], k, d, 2)
    assert out == CLEAN45
    assert [_row(x) for x in st] == [(3, 1, 0, 0), (2, 1, 0, 0)]
    # as ONE sequence the windows 20 .. 22 hold both errors, so no single change makes all windows
    # over either of them solid: the positions 22 .. 26 are candidates, none is accepted
    out, (one,) = correct(bad, [0, 45], k, d, 2)
    assert out == bad and _row(one) == (5, 0, 0, 0)
    # bytes outside [offsets[0], offsets[n]) are copied, positions outside are never candidates
    out, st = correct(bad, [25, 45], k, d, 2)
    assert out == bad[:25] + CLEAN45[25:] and [_row(x) for x in st] == [(2, 1, 0, 0)]


def _brute(text, offsets, k, d, solid_min):
    """The rule by its definition: no prefix sums, no shared helper."""
    s = max(solid_min, 1)
    comp = {65: 84, 67: 71, 71: 67, 84: 65}

    def T(w):
        w = w.upper()
        return d.get(min(w, bytes(comp[c] for c in reversed(w))), 0)

    def is_window(w, a, b):
        return a <= w and w + k <= b and all(c in b"ACGTacgt" for c in text[w:w + k])

    out, stats = bytearray(text), []
    for a, b in zip(offsets, offsets[1:]):
        st = dict.fromkeys(FIELDS, 0)
        acc = {}
        for p in range(a, b):
            C = [w for w in range(p - k + 1, p + 1) if is_window(w, a, b)]
            if text[p] not in b"ACGTacgt" or not C or any(T(text[w:w + k]) >= s for w in C):
                continue
            st["candidates"] += 1
            ys = [y for y in b"ACGT" if y != (text[p] & 0xDF) and
                  all(T(text[w:p] + bytes([y]) + text[p + 1:w + k]) >= s for w in C)]
            if len(ys) == 1:
                acc[p] = ys[0]
            elif ys:
                st["ambiguous"] += 1
        for p, y in acc.items():
            if [q for q in acc if q != p and abs(p - q) < k]:
                st["dropped"] += 1
            else:
                st["corrected"] += 1
                out[p] = y | (text[p] & 0x20)
        stats.append(st)
    return bytes(out), stats


def test_model_against_brute_force_and_the_output_properties():
    rng = random.Random(5)
    k = 9
    genome = bytes(rng.choice(b"ACGT") for _ in range(600))
    reads = [genome[p:p + 60] for p in range(0, 540, 7)]
    d = {}
    for r in reads:
        for p in range(len(r) - k + 1):
            c = canonical(r[p:p + k])
            d[c] = d.get(c, 0) + 1
    seqs = []
    for i, r in enumerate(reads[:40]):
        r = bytearray(r)
        for _ in range(rng.choice((0, 1, 1, 2))):
            p = rng.randrange(len(r))
            r[p] = rng.choice([c for c in b"ACGT" if c != r[p]])
        if i % 5 == 0:
            r[10:25] = bytes(r[10:25]).lower()
        if i % 7 == 0:
            r[rng.randrange(len(r))] = ord("N")
        seqs.append(bytes(r[:rng.choice((60, 60, 17, 9, 8, 0))]))
    text = b"".join(s + (b"\n" if i % 3 else b"") for i, s in enumerate(seqs))  # some joints without a break
    off = [0]
    for i, s in enumerate(seqs):
        off.append(off[-1] + len(s) + (1 if i % 3 else 0))
    for solid_min in (1, 2, 4):
        out, st = correct(text, off, k, d, solid_min)
        assert (out, st) == _brute(text, off, k, d, solid_min)
        assert guarantee_violations(text, out, off, k, d, solid_min) == []
    out, st = correct(text, off, k, d, 2)
    assert sum(x["corrected"] for x in st) >= 10 and sum(x["candidates"] - x["corrected"] for x in st) >= 10
    # the checker does notice what it is there to notice
    broken = bytearray(text)
    p = next(p for p in range(len(text)) if out[p] != text[p])
    broken[p] = ord("N")
    assert guarantee_violations(text, bytes(broken), off, k, d, 2)


def test_fields():
    assert correct_model.FIELDS == ("candidates", "corrected", "ambiguous", "dropped")
