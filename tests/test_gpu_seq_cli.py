"""GPU: the drop-in CLI's --coverage FILE --coverage-out FILE [--coverage-min N] -- per-record
statistics of the k-mer counts of a FASTA, FASTQ or one-sequence-per-line file -- next to an
unchanged counting run: the output file keeps the golden case's pinned digest.  Expected lines come
from the C oracle's -a 1 output through the pure-Python model of seq_model.py."""
import subprocess

import pytest

from conftest import CLI, load_cases, oracle_count, sorted_digest_file
import kaarme_amd as ka
import seq_model

pytestmark = pytest.mark.gpu


def _case(inp, k):
    for c in load_cases()["cases"]:
        if c["input"] == inp and c["k"] == k and "-b" not in c["args"] and "-m" not in c["args"] and \
                c["args"][:2] == ["-a", "2"]:
            return c
    raise KeyError((inp, k))


# the golden FASTA cases of test_gpu_query_cli.py, counted with the defaults (-m 2 -a 2)
CASES = [_case("big_skew.fasta", 31), _case("skew.fasta", 51)]


def _fasta_records(path):
    """[(name, sequence)]: the header's first token, the record's lines joined"""
    recs = []
    with open(path, "rb") as f:
        for line in f:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                recs.append([(line[1:].split() or [b""])[0].decode(), []])
            elif recs:
                recs[-1][1].append(line)
    return [(n, b"".join(p)) for n, p in recs]


def _model_lines(records, k, d, solid_min):
    text, off = ka.pack_sequences([s for _, s in records])
    st = seq_model.seq_stats(text, off, k, d, solid_min)
    return "".join("\t".join([n, str(len(s))] + [str(m[f]) for f in seq_model.FIELDS]) + "\n"
                   for (n, s), m in zip(records, st))


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c['input']}-k{c['k']}")
def test_cli_coverage(case, golden_input, tmp_path):
    path, k = golden_input(case["input"]), case["k"]
    exp = tmp_path / "oracle.txt"
    oracle_count(path, k, ["-m", "2", "-a", "1"], exp)
    d = seq_model.oracle_dict(exp)
    records = _fasta_records(path)
    slots = case["args"][case["args"].index("-s") + 1]
    base = [CLI, path, str(k), "-m", "2", "-a", "2", "-s", slots, "-t", "3"]
    # the input file itself; --coverage-min defaults to the -a value
    out, cov = tmp_path / "out.txt", tmp_path / "cov.tsv"
    r = subprocess.run(base + ["-o", str(out), "--coverage", path, "--coverage-out", str(cov)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert sorted_digest_file(str(out)) == (case["sorted_sha256"], case["lines"])  # unchanged behaviour
    assert f"({len(records)} coverage records)" in r.stdout
    assert cov.read_text() == _model_lines(records, k, d, 2)
    # 100 of its records as FASTQ, as plain text (names: line numbers; an empty line is no record)
    # and as FASTA wrapped at 60 columns with a described header and a record with an N
    some = records[::len(records) // 100][:100]
    some[3] = (some[3][0], some[3][1][:70] + b"N" + some[3][1][71:])
    fq, txt, fa = tmp_path / "some.fastq", tmp_path / "some.txt", tmp_path / "some.fa"
    fq.write_bytes(b"".join(b"@%s extra words\n%s\n+\n%s\n" % (n.encode(), s, b"I" * len(s)) for n, s in some))
    txt.write_bytes(b"".join(s + (b"\r\n" if i % 9 == 0 else b"\n") + (b"\n" if i == 4 else b"")
                             for i, (_, s) in enumerate(some)))
    fa.write_bytes(b"".join(b">%s\tdescribed\n" % n.encode() +
                            b"".join(s[i:i + 60] + b"\n" for i in range(0, len(s), 60)) for n, s in some))
    numbered = [(str(i + 1 + (i > 4)), s) for i, (_, s) in enumerate(some)]
    for src, recs, solid_min in ((fq, some, 5), (txt, numbered, 1), (fa, some, 16383)):
        r = subprocess.run(base + ["--digest-only", "--coverage", str(src), "--coverage-out", str(cov),
                                   "--coverage-min", str(solid_min)], capture_output=True, text=True, cwd=tmp_path)
        assert r.returncode == 0, r.stderr
        assert cov.read_text() == _model_lines(recs, k, d, solid_min), src.name


def test_cli_coverage_usage_errors(golden_input, tmp_path):
    path = golden_input("reads_w60.fasta")
    base = [CLI, path, "31", "-s", "100000", "-o", str(tmp_path / "out.txt")]
    r = subprocess.run(base + ["--coverage", path], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode != 0 and "--coverage requires --coverage-out" in r.stderr
    r = subprocess.run(base + ["--coverage-out", str(tmp_path / "c.tsv")], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode != 0 and "--coverage-out requires --coverage" in r.stderr
    # a missing file: nothing runs, nothing is written
    r = subprocess.run(base + ["--coverage", str(tmp_path / "nothing.fa"), "--coverage-out", str(tmp_path / "c.tsv")],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode != 0 and "nothing.fa" in r.stderr
    assert not (tmp_path / "c.tsv").exists() and not (tmp_path / "out.txt").exists()
