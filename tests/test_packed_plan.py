"""The sizing of a packed-stream pass (csrc/kc_plan_host.h) on the CPU.

tools/plan_host_check.cpp, built with the address and undefined-behaviour sanitizers, sweeps the
partition plan and the cut rule and replays heterogeneous streams through kc_count_packed_device's
batching: every batch's exact key buffers must hold the batch's true windows.  The same program
built with the parent's rule (the hint's density instead of the counted one) must fail there.

skm_model.packed_windows is the NumPy model of the window counter (kc_packed_windows_device): it
is checked here against sum(max(0, L - k + 1)) over the break-free runs and is the expected value
of tests/test_gpu_packed.py."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG
import skm_model as sm
from skm_model import packed_windows


def _formula(seqs, k):
    """sum of max(0, L - k + 1) over the maximal ACGT runs of the sequences"""
    n = 0
    for s in seqs:
        for run in "".join(c if c in "ACGTacgt" else " " for c in s).split():
            n += max(0, len(run) - k + 1)
    return n


def _build(target, *args):
    p = subprocess.run(["make", "-C", PKG, target, *args], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return os.path.join(PKG, target)


def test_plan_host_check_is_clean_under_the_sanitizers():
    exe = _build("bin/plan_host_check")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert " 0 failed" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr


def test_plan_host_check_fails_on_the_hint_density_rule():
    """Mutation check: with the windows hint's density sizing the buffers (what the pass did before
    it counted windows), the heterogeneous rows, and only they, must fail."""
    exe = _build("bin/plan_host_check_mutant", "PLANSUFFIX=_mutant", "PLANFLAGS=-DKC_PLAN_MUTANT_HINT_DENSITY")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 1, p.stdout + p.stderr
    fails = [l for l in p.stdout.splitlines() if l.startswith("FAIL")]
    assert fails and all("heterogeneous" in l for l in fails), p.stdout
    assert any("need1 >= wins" in l for l in fails), p.stdout


RNG = np.random.default_rng(5)


def _seq(n):
    return "".join("ACGT"[i] for i in RNG.integers(0, 4, n))


K = 31
CASES = {
    "empty": [],
    "shorter_than_k": [_seq(K - 1), _seq(1), _seq(K - 1)],
    "exactly_k": [_seq(K), _seq(K), _seq(K - 1), _seq(K)],
    "consecutive_breaks": [_seq(40) + "NNN" + _seq(K) + "N" + "N" + _seq(K + 1), "", "", _seq(33)],
    # the break + 31 symbols fill word 0: the run ends at the word's last symbol (bit 0)
    "run_ends_at_bit_0": [_seq(31), _seq(63), _seq(5)],
    # 31 symbols, then N x 32: the last word is nothing but breaks (the N run), then padding
    "last_word_all_padding": [_seq(31) + "N" * 32],
    "long_run": [_seq(1000)],
    "mixed": [_seq(int(n)) for n in RNG.integers(1, 200, 60)],
}


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("k", [1, 5, 31, 32, 33, 51, 127, 479])
def test_window_model_matches_the_run_formula(name, k):
    seqs = CASES[name]
    pk, bk = sm.pack(seqs)
    assert packed_windows(bk, k) == _formula(seqs, k)
    # a whole word of padding breaks appended changes nothing
    assert packed_windows(np.concatenate([bk, np.array([0xFFFFFFFF], np.uint32)]), k) == _formula(seqs, k)


def test_window_model_edge_layouts():
    pk, bk = sm.pack(CASES["run_ends_at_bit_0"])
    assert bk[0] == 0x80000000 and bk[1] == 0x80000000  # word 0: break + 31 symbols; the next starts a run
    pk, bk = sm.pack(CASES["last_word_all_padding"])
    assert bk[-1] == 0xFFFFFFFF and len(bk) == 2
    # a sub-range that starts inside a run sees only what lies inside it
    pk, bk = sm.pack([_seq(200)])
    assert packed_windows(bk, 31) == 170
    assert packed_windows(bk[1:], 31) == 200 + 1 - 32 - 30
    assert packed_windows(bk[:2], 31) == 63 - 30


def test_window_model_agrees_with_a_scalar_loop():
    bk = RNG.integers(0, 1 << 32, 300, dtype=np.uint64).astype(np.uint32)
    bk[RNG.integers(0, 300, 200)] = 0  # (random words are break-dense: some runs of whole words)
    for k in (1, 2, 7, 33, 70):
        n = run = 0
        for w in bk:
            for j in range(32):
                run = 0 if (int(w) >> (31 - j)) & 1 else run + 1
                n += run >= k
        assert packed_windows(bk, k) == n
