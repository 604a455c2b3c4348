"""CPU: the slot tags and tag-word masks of level 3's insert (csrc/kc_slot_mask.h, the code k_p3 runs)
against a byte-by-byte loop.

tools/slot_mask_check.cpp, built with the address and undefined-behaviour sanitizers, sweeps every
bucket size S in {1, 2, 3, 4, 5, 8}, every tag and every tag word over {0, tag, tag ^ 1, 0x80, 0xFF}: the
match mask and the empty mask, walked by first / rest, must list the slots the loop lists.  The same
program with the constant of a bucket's first S bytes one byte off must fail."""
import os
import re
import subprocess

from conftest import PKG


def _build(target, *args):
    p = subprocess.run(["make", "-C", PKG, target, *args], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    return os.path.join(PKG, target)


def _figures(text):
    m = re.search(r"(\d+) checked, (\d+) with a match, (\d+) with an empty slot, (\d+) failed", text)
    assert m, text
    return dict(zip(("checked", "matches", "empties", "failed"), map(int, m.groups())))


def test_slot_mask_check_is_clean_under_the_sanitizers():
    exe = _build("bin/slot_mask_check")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr
    f = _figures(p.stdout)
    assert f["failed"] == 0 and f["checked"] == 6 * 255 * 5 ** 8
    assert 0 < f["matches"] < f["checked"] and 0 < f["empties"] < f["checked"]


def test_slot_mask_check_fails_on_a_constant_one_byte_off():
    """Mutation check: with one byte more (S = 8: one less) in the S-byte constant, slots beyond the
    bucket are listed, or its last slot is not."""
    exe = _build("bin/slot_mask_check_mutant", "SLOTSUFFIX=_mutant", "SLOTFLAGS=-DKC_SLOT_MUTANT_SMASK")
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 1, p.stdout + p.stderr
    f = _figures(p.stdout)
    assert f["failed"] > 1000000
