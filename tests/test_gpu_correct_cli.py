"""GPU: the drop-in CLI's --correct FILE --correct-out FILE [--correct-min N] -- the records of a
FASTA, FASTQ or one-sequence-per-line file with their isolated base errors corrected from the table,
written back in the file's format -- next to an unchanged counting run: the output file keeps the
golden case's pinned digest.  Expected records come from the C oracle's -a 1 output through the
pure-Python model of correct_model.py."""
import gzip
import subprocess

import pytest

from conftest import CLI, load_cases, oracle_count, sorted_digest_file
import kaarme_amd as ka
import correct_model
import seq_model

pytestmark = pytest.mark.gpu


def _case(inp, k):
    for c in load_cases()["cases"]:
        if c["input"] == inp and c["k"] == k and "-b" not in c["args"] and "-m" not in c["args"] and \
                c["args"][:2] == ["-a", "2"]:
            return c
    raise KeyError((inp, k))


CASE = _case("big_skew.fasta", 31)  # counted with the defaults (-m 2 -a 2), as test_gpu_seq_cli.py


def _fasta_records(path):
    """[(header line, sequence)]: the record's lines joined"""
    recs = []
    with open(path, "rb") as f:
        for line in f:
            line = line.rstrip(b"\r\n")
            if line.startswith(b">"):
                recs.append([line, []])
            elif recs:
                recs[-1][1].append(line)
    return [(h, b"".join(p)) for h, p in recs]


def _plant(seq, p):
    return seq[:p] + b"CGTA"[b"ACGT".index(seq[p:p + 1].upper()):][:1] + seq[p + 1:]


def _model(seqs, k, d, solid_min):
    text, off = ka.pack_sequences(seqs)
    out, st = correct_model.correct(text, off, k, d, solid_min)
    fixed = [out[int(off[i]):int(off[i + 1]) - 1] for i in range(len(seqs))]
    tot = {f: sum(s[f] for s in st) for f in correct_model.FIELDS}
    line = "Corrected %d bases in %d of %d records (%d candidates, %d ambiguous, %d dropped)" % (
        tot["corrected"], sum(s["corrected"] > 0 for s in st), len(seqs), tot["candidates"], tot["ambiguous"],
        tot["dropped"])
    return fixed, line, tot


def test_cli_correct(golden_input, tmp_path):
    path, k = golden_input(CASE["input"]), CASE["k"]
    exp = tmp_path / "oracle.txt"
    oracle_count(path, k, ["-m", "2", "-a", "1"], exp)
    d = seq_model.oracle_dict(exp)
    records = _fasta_records(path)
    some = [(b">" + h[1:].split()[0] + b"\tdescribed  twice", s) for h, s in records[::len(records) // 100][:100]]
    some = [(h, _plant(s, len(s) // 2) if i % 2 and len(s) >= k else s) for i, (h, s) in enumerate(some)]
    some[3] = (some[3][0], some[3][1][:70] + b"N" + some[3][1][71:])
    some[6] = (some[6][0], some[6][1][:40].lower() + some[6][1][40:])
    some[8] = (some[8][0], b"")  # an empty record
    seqs = [s for _, s in some]
    slots = CASE["args"][CASE["args"].index("-s") + 1]
    base = [CLI, path, str(k), "-m", "2", "-a", "2", "-s", slots, "-t", "3"]
    fa, fq, txt = tmp_path / "some.fa", tmp_path / "some.fastq", tmp_path / "some.txt"
    fa.write_bytes(b"".join(h + (b"\r\n" if i % 4 == 0 else b"\n") +
                            b"".join(s[j:j + 60] + (b"\r\n" if i % 4 == 0 else b"\n") for j in range(0, len(s), 60))
                            for i, (h, s) in enumerate(some)))
    quals = [(b"@" if i % 3 == 0 and s else b"") + b"I" * (len(s) - (1 if i % 3 == 0 and s else 0)) for i, s in enumerate(seqs)]
    fq.write_bytes(b"".join(b"@" + h[1:] + b"\n" + s + b"\n+" + (h[1:] if i % 5 == 0 else b"") + b"\n" + q + b"\n"
                            for i, ((h, s), q) in enumerate(zip(some, quals))))
    plain = [s for s in seqs if s]
    txt.write_bytes(b"".join(s + (b"\r\n" if i % 9 == 0 else b"\n") + (b"\n" if i == 4 else b"")
                             for i, s in enumerate(plain)))
    out, res = tmp_path / "out.txt", tmp_path / "fixed.out"

    # FASTA, next to the counting run and its output file; --correct-min defaults to the -a value
    fixed, line, tot = _model(seqs, k, d, 2)
    assert tot["corrected"] >= 10
    r = subprocess.run(base + ["-o", str(out), "--correct", str(fa), "--correct-out", str(res)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert sorted_digest_file(str(out)) == (CASE["sorted_sha256"], CASE["lines"])  # unchanged behaviour
    assert line in r.stdout.splitlines()
    assert res.read_bytes() == b"".join(h + b"\n" + s + b"\n" for (h, _), s in zip(some, fixed))
    # FASTQ (a quality line that starts with '@', '+' lines that repeat the name), with --coverage beside it
    fixed, line, tot = _model(seqs, k, d, 1)
    assert tot["corrected"] >= 10
    r = subprocess.run(base + ["--digest-only", "--correct", str(fq), "--correct-out", str(res), "--correct-min", "1",
                               "--coverage", str(fq), "--coverage-out", str(tmp_path / "cov.tsv")],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert line in r.stdout.splitlines()
    assert res.read_bytes() == b"".join(b"@" + h[1:] + b"\n" + s + b"\n+" + (h[1:] if i % 5 == 0 else b"") + b"\n" + q + b"\n"
                                        for i, ((h, _), s, q) in enumerate(zip(some, fixed, quals)))
    assert len((tmp_path / "cov.tsv").read_text().splitlines()) == len(some)
    # one sequence per line (an empty line is no record)
    fixed, line, tot = _model(plain, k, d, 3)
    r = subprocess.run(base + ["--digest-only", "--correct", str(txt), "--correct-out", str(res), "--correct-min", "3"],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert line in r.stdout.splitlines()
    assert res.read_bytes() == b"".join(s + b"\n" for s in fixed)


def test_cli_correct_against_an_op_result(golden_input, tmp_path):
    """With --op the correction reads the resulting table: intersect-min of the input with itself
    holds the input's counts."""
    path, k = golden_input(CASE["input"]), CASE["k"]
    exp = tmp_path / "oracle.txt"
    oracle_count(path, k, ["-m", "2", "-a", "1"], exp)
    d = seq_model.oracle_dict(exp)
    seqs = [_plant(s, 50) for _, s in _fasta_records(path)[:40]]
    txt, res = tmp_path / "r.txt", tmp_path / "r.out"
    txt.write_bytes(b"".join(s + b"\n" for s in seqs))
    fixed, line, tot = _model(seqs, k, d, 2)
    slots = CASE["args"][CASE["args"].index("-s") + 1]
    r = subprocess.run([CLI, path, str(k), "-s", slots, "--digest-only", "--op", "intersect-min", "--with", path,
                        "--correct", str(txt), "--correct-out", str(res)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    assert line in r.stdout.splitlines()
    assert res.read_bytes() == b"".join(s + b"\n" for s in fixed)


def test_cli_correct_usage_errors(golden_input, tmp_path):
    path = golden_input("reads_w60.fasta")
    base = [CLI, path, "31", "-s", "100000", "-o", str(tmp_path / "out.txt")]
    res = tmp_path / "c.out"

    def run(*extra):
        return subprocess.run(base + list(extra), capture_output=True, text=True, cwd=tmp_path)

    r = run("--correct", path)
    assert r.returncode != 0 and "--correct requires --correct-out" in r.stderr
    r = run("--correct-out", str(res))
    assert r.returncode != 0 and "--correct-out requires --correct" in r.stderr
    r = run("--correct-min", "3")
    assert r.returncode != 0 and "--correct-min requires --correct" in r.stderr
    # a missing, a gzip and an ill-formed file: nothing runs, nothing is written
    r = run("--correct", str(tmp_path / "nothing.fa"), "--correct-out", str(res))
    assert r.returncode != 0 and "nothing.fa" in r.stderr
    gz = tmp_path / "r.fa.gz"
    gz.write_bytes(gzip.compress(b">r\nACGT\n"))
    r = run("--correct", str(gz), "--correct-out", str(res))
    assert r.returncode != 0 and "gzip input is not supported" in r.stderr
    bad = tmp_path / "bad.fa"
    bad.write_bytes(b"ACGT\n")
    r = run("--correct", str(bad), "--correct-out", str(res))
    assert r.returncode != 0 and "ill-formed" in r.stderr
    assert not res.exists() and not (tmp_path / "out.txt").exists()
    assert "--correct-out" in subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout
