"""CPU: the comparison of weak-link removal's rule (csrc/kc_weak_rule.h, the code k_weak_verdict runs)
against 128-bit integers.

T(c) is below 2^16 in every count mode, so on a graph that a GPU test can hold the rule's two products
stay below 2^64 (weak_cases.big_counts reaches 2^35).  tools/weak_rule_check.cpp, built with the
address and undefined-behaviour sanitizers, sweeps the header's own arithmetic up to the largest
values include/kc_api.h allows -- sides above 2^64, equal sides, sides one count apart.  The same
program with its reference cut to 64 bits must fail, on exactly the inputs where 64 bits give the
other verdict."""
import os
import re
import subprocess

from conftest import PKG


def _build(target, *args):
    p = subprocess.run(["make", "-C", PKG, target, *args], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return os.path.join(PKG, target)


def _figures(text):
    m = re.search(r"(\d+) checked, (\d+) with a side above 2\^64, (\d+) where 64 bits give the other verdict, (\d+) weak, "
                  r"(\d+) failed", text)
    assert m, text
    return dict(zip(("checked", "wide", "flips64", "weak", "failed"), map(int, m.groups())))


def test_weak_rule_check_is_clean_under_the_sanitizers():
    exe = _build("bin/weak_rule_check")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
    f = _figures(p.stdout)
    assert f["failed"] == 0 and f["checked"] > 1000000 and f["wide"] > 100000 and f["flips64"] > 1000
    assert 0 < f["weak"] < f["checked"]


def test_weak_rule_check_fails_on_a_64_bit_reference():
    """Mutation check: against products cut to 64 bits, the header's answers differ exactly where the
    cut changes the verdict."""
    exe = _build("bin/weak_rule_check_mutant", "WEAKSUFFIX=_mutant", "WEAKFLAGS=-DKC_WEAK_MUTANT_64")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 1, p.stdout + p.stderr
    f = _figures(p.stdout)
    assert f["failed"] == f["flips64"] > 1000
