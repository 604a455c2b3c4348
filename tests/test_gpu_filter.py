"""GPU: what graph cleaning (kc_clean*) and bubble popping (kc_pop_bubbles*) share, the host path of
kc_api_filter.cpp, and the error routing they share with the table algebra (kc_table_op*).

With their rules off both filters are the same call: the copy of src's range into dst, with the
range's unitig and node totals.  Expected = the two pure-Python models on the source's own dump()."""
import ctypes

import pytest

import bubble_cases as bc
import bubble_model as bm
import clean_cases as cc
import clean_model as clm
import kaarme_amd as ka
from test_gpu_clean import fresh
from test_gpu_graph import count, same, table_of

pytestmark = pytest.mark.gpu

KC_ERR_ARG = -1
RANGES = [(1, 0), (2, 0), (1, 3)]
SHARED = ("unitigs", "nodes", "out_keys", "out_sum")


@pytest.fixture(scope="module")
def counted():
    """k -> (counter of bubble_cases.variants(k), its table as a dict), made once"""
    made = {}

    def get(k):
        if k not in made:
            kc = count(cc.fasta(bc.variants(k)[0]), k, table_slots=1 << 14)
            made[k] = (kc, table_of(kc))
        return made[k]

    yield get
    for kc, _ in made.values():
        kc.close()


# ---- 1. both filters with their rules off are the same copy ----------------------------------------
@pytest.mark.parametrize("k,distinct", [(31, 619), (32, 639)])
def test_rules_off_both_filters_copy_the_range(k, distinct, counted):
    src, table = counted(k)
    assert len(table) == distinct
    before = (src.output_digest(), src.finish())
    for lo, hi in RANGES:
        in_range = {c: v for c, v in table.items() if v >= lo and (hi == 0 or v <= hi)}
        want_c, st_c = clm.clean(table, lo, hi)
        want_p, st_p = bm.pop(table, lo, hi)
        assert want_c == want_p == in_range and 0 < len(in_range)
        if (k, lo, hi) == (31, 2, 0):
            assert (st_c["unitigs"], st_c["nodes"], st_c["out_sum"]) == (1, 465, 1405)
        with fresh(k, 1 << 14) as cleaned, fresh(k, 1 << 14) as popped:
            got_c = cleaned.clean(src, lo, hi)
            got_p = popped.pop_bubbles(src, lo, hi)
            for f in SHARED:
                assert got_c[f] == got_p[f] == st_c[f] == st_p[f], (k, lo, hi, f, got_c, got_p, st_c, st_p)
            assert got_c == st_c and got_p == st_p
            ok = same(table_of(cleaned), in_range) and same(table_of(popped), in_range)
            assert ok, (k, lo, hi)
    assert (src.output_digest(), src.finish()) == before
    ok = same(table_of(src), table)
    assert ok


# ---- 2. the error lands on the context the caller reads --------------------------------------------
CALLS = {
    "kc_table_op": (lambda: ka.kc_op_desc(ka.OP_SUBTRACT, 3, 2, 1, 0, 0), 2, b"kc_table_op: a range's min is above its max"),
    "kc_clean": (lambda: ka.kc_clean_desc(3, 2, 0, 0, 0, 0), 1, b"min_count is above max_count"),
    "kc_pop_bubbles": (lambda: ka.kc_bubble_desc(3, 2, 0, 0, 0, 0), 1, b"min_count is above max_count"),
}


@pytest.mark.parametrize("device_form", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("call", list(CALLS))
def test_error_lands_on_the_context_the_caller_reads(call, device_form, counted):
    src, table = counted(31)
    make_desc, operands, message = CALLS[call]
    desc = make_desc()
    lib = src.lib
    fn = getattr(lib, call + ("_device" if device_form else ""))
    tail = (None, None) if device_form else (None,)  # no statistics (, the null stream)
    with fresh(31, 1 << 14) as dst, count(cc.fasta(bc.variants(31)[0][:1]), 31, table_slots=1 << 14) as first:
        ops = [first._ctx] + [src._ctx] * (operands - 1)
        assert message not in lib.kc_last_error(dst._ctx) and message not in lib.kc_last_error(first._ctx)
        assert fn(None, *ops, ctypes.byref(desc), *tail) == KC_ERR_ARG
        assert message in lib.kc_last_error(first._ctx) and message not in lib.kc_last_error(dst._ctx)
        assert fn(dst._ctx, *ops, ctypes.byref(desc), *tail) == KC_ERR_ARG
        assert message in lib.kc_last_error(dst._ctx)
        # the refused calls changed nothing
        assert table_of(dst) == {} and dst.finish()["inserted"] == 0
    ok = same(table_of(src), table)
    assert ok
