"""Pure-Python model of the read correction (kc_correct*), the rule of include/kc_api.h over a
{canonical k-mer: T(c)} dictionary (the C oracle's ``-a 1`` output through seq_model.oracle_dict).
Independent of the code under test.

For sequence i = text[a:b], s = max(solid_min, 1):
  windows       w with a <= w, w + k <= b, text[w:w+k] all bases
  C(p)          the windows with w <= p < w + k
  candidate(p)  C(p) is not empty and every window of it has T < s
  works(p, y)   y another base: every window of C(p) with byte p replaced by y has T >= s
  accepted(p)   candidate and exactly one y works;  ambiguous(p): two or three work
  dropped(p)    accepted, and another accepted q of the sequence has |p - q| < k
  out[p]        the working y in text[p]'s letter case if accepted and not dropped, else text[p]
"""
from seq_model import NO_KMER, canonical, text_counts

FIELDS = ("candidates", "corrected", "ambiguous", "dropped")
_BASES = (b"A", b"C", b"G", b"T")


def correct(text: bytes, offsets, k: int, d: dict, solid_min: int = 1):
    """(the corrected text, one {FIELDS} dict per sequence [offsets[i], offsets[i + 1]))."""
    s = max(int(solid_min), 1)
    off = [int(o) for o in offsets]
    out = bytearray(text)
    stats = []
    for a, b in zip(off, off[1:]):
        st = dict.fromkeys(FIELDS, 0)
        stats.append(st)
        if b - a < k:
            continue
        cnt = text_counts(text, k, d, a, b)[:b - a - k + 1]  # cnt[w - a] of the window starts a .. b - k
        valid, solid = [0], [0]  # prefix counts: windows a .. a + j - 1 that exist / that are solid
        for c in cnt:
            valid.append(valid[-1] + (c != NO_KMER))
            solid.append(solid[-1] + (c != NO_KMER and c >= s))
        accepted = {}
        for p in range(a, b):
            lo, hi = max(a, p - k + 1), min(p, b - k)  # the window starts that can hold p
            if valid[hi + 1 - a] == valid[lo - a] or solid[hi + 1 - a] != solid[lo - a]:
                continue
            st["candidates"] += 1
            cover = [w for w in range(lo, hi + 1) if cnt[w - a] != NO_KMER]
            have = text[p:p + 1].upper()
            works = [y for y in _BASES if y != have and
                     all(d.get(canonical((text[w:p] + y + text[p + 1:w + k]).upper()), 0) >= s for w in cover)]
            if len(works) == 1:
                accepted[p] = works[0]
            elif works:
                st["ambiguous"] += 1
        for p, y in accepted.items():
            if any(q != p and abs(q - p) < k for q in accepted):
                st["dropped"] += 1
            else:
                st["corrected"] += 1
                out[p] = ord(y) | (text[p] & 0x20)  # the letter case of text[p]
    return bytes(out), stats


def guarantee_violations(text: bytes, out: bytes, offsets, k: int, d: dict, solid_min: int = 1) -> list:
    """What an output must never show: a byte changed into something that is no other base of the
    same letter case, a changed byte outside every sequence, or a window (of a sequence) that holds a
    changed byte and is not solid in d.  (A window without a changed byte is the input's, given the
    first.)  Returns descriptions; [] is a pass."""
    s = max(int(solid_min), 1)
    bad = []
    if len(out) != len(text):
        return ["length"]
    changed = [p for p in range(len(text)) if out[p] != text[p]]
    for p in changed:
        if text[p:p + 1].upper() not in _BASES or out[p:p + 1].upper() not in _BASES or (text[p] ^ out[p]) & 0x20:
            bad.append(("byte", p))
    off = [int(o) for o in offsets]
    inside = set()
    for a, b in zip(off, off[1:]):
        here = [p for p in changed if a <= p < b]
        inside.update(here)
        if not here:
            continue
        cnt = text_counts(out, k, d, a, b)
        for p in here:
            ws = [w for w in range(max(a, p - k + 1), min(p, b - k) + 1) if cnt[w - a] != NO_KMER]
            if not ws:
                bad.append(("no window", p))
            bad += [("weak window", w) for w in ws if cnt[w - a] < s]
            if any(q != p and abs(q - p) < k for q in here):
                bad.append(("two changes in a window", p))
    bad += [("outside", p) for p in changed if p not in inside]
    return bad
