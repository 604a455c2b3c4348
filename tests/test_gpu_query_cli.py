"""GPU: the drop-in CLI's query extensions -- --histo FILE (the abundance spectrum) and
--query FILE --query-out FILE (one k-mer per line, either strand, any case) -- next to an unchanged
counting run: the output file keeps the golden case's pinned digest."""
import subprocess

import numpy as np
import pytest

from conftest import CLI, load_cases, oracle_count, sorted_digest_file

pytestmark = pytest.mark.gpu


def _case(inp, k):
    for c in load_cases()["cases"]:
        if c["input"] == inp and c["k"] == k and "-b" not in c["args"] and "-m" not in c["args"] and \
                c["args"][:2] == ["-a", "2"]:
            return c
    raise KeyError((inp, k))


# golden FASTA cases counted with the defaults the test passes explicitly (-m 2 -a 2)
CASES = [_case("big_skew.fasta", 31), _case("skew.fasta", 51)]
COMP = str.maketrans("ACGT", "TGCA")


def _revcomp(s):
    return s.translate(COMP)[::-1]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c['input']}-k{c['k']}")
def test_cli_histo_and_query(case, golden_input, tmp_path):
    path, k = golden_input(case["input"]), case["k"]
    exp = tmp_path / "oracle.txt"
    oracle_count(path, k, ["-m", "2", "-a", "1"], exp)
    table = {}
    with open(exp) as f:
        for line in f:
            s, c = line.split()
            table[s] = int(c)
    kmers = list(table)
    rng = np.random.default_rng(k)
    some = [kmers[i] for i in rng.choice(len(kmers), size=300, replace=False)]
    absent = []
    while len(absent) < 20:
        s = "".join(rng.choice(list("ACGT"), size=k))
        if s not in table and _revcomp(s) not in table:
            absent.append(s)
    with_n = some[0][:k // 2] + "N" + some[0][k // 2 + 1:]
    queries = some + [_revcomp(s) for s in some] + [s.lower() for s in some] + absent + [with_n]
    want = [table[s] for s in some] * 3 + [0] * 21
    q = tmp_path / "q.txt"
    # (CRLF and empty lines are tolerated)
    q.write_text("".join(s + ("\r\n" if i % 7 == 0 else "\n") + ("\n" if i % 50 == 0 else "") for i, s in enumerate(queries)))
    out, h, a = tmp_path / "out.txt", tmp_path / "h.txt", tmp_path / "a.txt"
    slots = case["args"][case["args"].index("-s") + 1]
    r = subprocess.run([CLI, path, str(k), "-m", "2", "-a", "2", "-s", slots, "-t", "3", "-o", str(out), "--histo", str(h),
                        "--query", str(q), "--query-out", str(a)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert sorted_digest_file(str(out)) == (case["sorted_sha256"], case["lines"])  # unchanged behaviour
    spectrum = np.bincount(np.array(list(table.values()), dtype=np.int64))
    assert h.read_text() == "".join(f"{v} {n}\n" for v, n in enumerate(spectrum.tolist()) if n)
    assert a.read_text() == "".join(f"{s} {c}\n" for s, c in zip(queries, want))
    # without -o and with --digest-only: the same answers
    r = subprocess.run([CLI, path, str(k), "-m", "2", "-a", "2", "-s", slots, "-t", "3", "--digest-only", "--histo", str(h),
                        "--query", str(q), "--query-out", str(a)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert "Output digest:" in r.stdout
    assert a.read_text() == "".join(f"{s} {c}\n" for s, c in zip(queries, want))


def test_cli_query_usage_errors(golden_input, tmp_path):
    path = golden_input("reads_w60.fasta")
    q = tmp_path / "q.txt"
    q.write_text("A" * 31 + "\n\n" + "C" * 30 + "\n")
    r = subprocess.run([CLI, path, "31", "-s", "100000", "--query", str(q), "--query-out", str(tmp_path / "a.txt")],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode != 0
    assert "line 3" in r.stderr
    assert not (tmp_path / "a.txt").exists()
    q.write_text("A" * 31 + "\n")
    r = subprocess.run([CLI, path, "31", "-s", "100000", "--query", str(q)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode != 0
    assert "--query requires --query-out" in r.stderr
