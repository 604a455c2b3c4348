"""CPU: the table of key widths (key_widths.py) reaches all fifteen widths and all six bucket shapes in
every kernel family, so that no width drops out of the suite unseen; and the C oracle against a plain
Python dictionary count at the widths W = 11 and 13, both ends of each."""
import re

import pytest

import graph_model
import kaarme_amd as ka
import key_widths as kw
from conftest import load_cases, oracle_count

ALL = set(range(1, 16))


def test_both_ends_of_every_width():
    assert {ka.words_for_k(k) for k in kw.K_HI.values()} == ALL
    assert {ka.words_for_k(k) for k in kw.K_LO.values()} == ALL
    for W in ALL:
        assert ka.words_for_k(kw.K_HI[W]) == ka.words_for_k(kw.K_LO[W]) == W
        assert kw.K_HI[W] % 32 == 31 and (kw.K_LO[W] % 32 == 0 or W == 1)
    # one k more is the next width, one less than the narrow end the one before
    assert all(ka.words_for_k(kw.K_HI[W] + 1) == W + 1 and ka.words_for_k(kw.K_LO[W] - 1) == max(W - 1, 1) for W in ALL)
    assert max(kw.K_HI.values()) == 479  # the widest key the engine takes


def test_all_six_bucket_shapes():
    shapes = {W: kw.slots_per_bucket(W) for W in ALL}
    assert set(shapes.values()) == {8, 5, 4, 3, 2, 1}
    assert [shapes[W] for W in (1, 2, 3, 4, 5, 6, 7, 8, 15)] == [8, 5, 4, 3, 2, 2, 2, 1, 1]
    # the spare words of a bucket: none at W = 1, 3, 7, 15, four at 5, seven at 8
    spare = {W: 16 - shapes[W] * (W + 1) for W in ALL}
    assert [spare[W] for W in (1, 2, 3, 4, 5, 6, 7, 8, 15)] == [0, 1, 0, 1, 4, 2, 0, 7, 0]
    assert [shapes[W] for W in kw.HEAVY_LO_WIDTHS] == [3, 2, 2, 1] and [spare[W] for W in kw.HEAVY_LO_WIDTHS] == [1, 4, 0, 7]


def test_every_family_list_covers_every_width():
    assert kw.widths_of(kw.CHEAP_KS) == ALL and len(kw.CHEAP_KS) == 30
    assert kw.widths_of(kw.HEAVY_KS) == ALL and len(kw.HEAVY_KS) == 19
    assert set(kw.HEAVY_KS) <= set(kw.CHEAP_KS)
    assert {kw.K_LO[W] for W in kw.HEAVY_LO_WIDTHS} <= set(kw.HEAVY_KS)
    # the older files and the new one together, family by family
    for family, new in kw.NEW_KS.items():
        assert kw.widths_of(new) | kw.widths_of(kw.OLD_KS.get(family, [])) == ALL, family
    assert set(kw.HEAVY_NEW_KS) | set(kw.HEAVY_OLD_KS) == set(kw.HEAVY_KS)
    for family in ("neighbors, graph", "unitigs", "table_op"):
        assert set(kw.HEAVY_OLD_KS) <= set(kw.OLD_KS[family]), family
    # every width has an input
    for k in kw.CHEAP_KS:
        assert k <= 65 or k >= 95
    # the unsampled distinct-count sketch is the one of keys of five words and more
    assert kw.widths_of(kw.HLL_KS) == {5, 8, 11, 13, 15}
    assert kw.widths_of(kw.UNPINNED_KS) == {11, 13} and set(kw.UNPINNED_KS) == {kw.K_LO[11], kw.K_HI[11], kw.K_LO[13], kw.K_HI[13]}


def test_reference_fixtures_cover_every_width():
    """counting (three insert paths, test_gpu_parity.py) and the compact representation
    (test_gpu_compact.py) run the golden cases: every width has one, and the two widths that had
    none have one that the compact test takes (no Bloom filter, not -m 0), too"""
    cases = load_cases()["cases"]
    assert kw.widths_of(c["k"] for c in cases) == ALL
    compact = [c for c in cases if "-b" not in c["args"] and ("-m" not in c["args"] or c["args"][c["args"].index("-m") + 1] != "0")]
    assert {11, 13} <= kw.widths_of(c["k"] for c in compact)
    for k in (kw.K_HI[11], kw.K_HI[13]):
        mine = [c["args"] for c in cases if c["k"] == k and c["input"] == "long_lo.fasta"]
        assert ["-a", "1", "-s", "1000000"] in mine and ["-b", "-u", "300000", "-a", "2"] in mine


def _dictionary_count(path, k):
    """{canonical k-mer: min(count, 16383)} of the sequence lines of a FASTA file, the plain way"""
    counts = {}
    with open(path) as f:
        for line in f:
            if line.startswith(">"):
                continue
            for run in re.findall("[ACGT]+", line.upper()):
                for p in range(len(run) - k + 1):
                    c = graph_model.canon(run[p:p + k])
                    counts[c] = counts.get(c, 0) + 1
    return {c: min(n, 16383) for c, n in counts.items()}


@pytest.mark.parametrize("k", kw.UNPINNED_KS)
def test_oracle_equals_a_dictionary_count(k, golden_input, tmp_path):
    """The oracle is pinned by reference fixtures at k = 351 and 415 only from this table on, and at no
    k with an empty top word in W = 11 and 13: here its -a 1 lines are a Python dictionary's."""
    path = golden_input("long_lo.fasta")
    out = tmp_path / "o.txt"
    st = oracle_count(path, k, ["-m", "2", "-a", "1"], out)
    with open(out) as f:
        lines = [line.split() for line in f]
    got = {s: int(c) for s, c in lines}
    want = _dictionary_count(path, k)
    assert len(got) == len(lines) == st["distinct"] and all(len(s) == k for s in got)
    assert len(want) > 50000 and max(want.values()) >= 2
    assert got == want
