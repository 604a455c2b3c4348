"""The one table of key widths of the width tests (test_key_widths.py on the CPU, test_gpu_key_widths.py
on the GPU).

A key of k bases takes W = k // 32 + 1 64-bit words, W = 1 .. 15; every device path that touches the
table is compiled once per W, and a 128-byte bucket holds S = 16 // (W + 1) slots, so the bucket
shape, the probe form, the record format and the thread counts all change with W.  For every W two
values of k stand for it:
  K_HI[W] = 32 W - 1     the top word holds 31 bases (the widest key of W words)
  K_LO[W] = 32 (W - 1)   the top word holds no base at all (the narrowest; K_LO[1] = 5)
and the lists below say which of them each kernel family runs."""
import kaarme_amd as ka
import test_gpu_correct
import test_gpu_graph
import test_gpu_query
import test_gpu_seq
import test_gpu_tableop
import test_gpu_unitig

WIDTHS = range(1, 16)
K_HI = {W: 32 * W - 1 for W in WIDTHS}
K_LO = {W: 32 * (W - 1) if W > 1 else 5 for W in WIDTHS}


def slots_per_bucket(W):
    """the slots of (W key words + 1 count word) of a 16-word bucket"""
    return 16 // (W + 1)


def widths_of(ks):
    """the set of key widths a list of k reaches"""
    return {ka.words_for_k(k) for k in ks}


# lookup, histogram, text_counts, seq_stats, compact + compact_lookup + compact_dump (and the counting
# itself, against the oracle): both ends of every width
CHEAP_KS = sorted(set(K_HI.values()) | set(K_LO.values()))
# neighbors, graph, unitigs, table_op, correct (Python models of seconds per k): the wide end of every
# width, and the narrow end of the three-slot bucket (W = 4), the two-slot bucket with four spare
# words (5) and with none (7), and the first one-slot bucket (8)
HEAVY_LO_WIDTHS = (4, 5, 7, 8)
HEAVY_KS = sorted(set(K_HI.values()) | {K_LO[W] for W in HEAVY_LO_WIDTHS})
# ... of which test_gpu_key_widths.py runs the ones that test_gpu_graph.py, test_gpu_unitig.py and
# test_gpu_tableop.py (one list in all three) do not run already
HEAVY_OLD_KS = sorted(set(test_gpu_graph.KS) & set(test_gpu_unitig.KS) & set(test_gpu_tableop.KS) & set(HEAVY_KS))
HEAVY_NEW_KS = [k for k in HEAVY_KS if k not in HEAVY_OLD_KS]
# kc_estimate_distinct_device past four words: the unsampled k_hll<W> (test_gpu_parity.py runs the sampled one)
HLL_KS = [128, 255, 320, 415, 479]
# both ends of the two widths that no reference fixture reached before (W = 11, 13)
UNPINNED_KS = [320, 351, 384, 415]

# what the older files run, family by family (the union with the lists above is checked on the CPU)
OLD_KS = {
    "lookup, histogram": test_gpu_query.KS,
    "text_counts": test_gpu_seq.KS,
    "correct": test_gpu_correct.KS,
    "neighbors, graph": test_gpu_graph.KS,
    "unitigs": test_gpu_unitig.KS,
    "table_op": test_gpu_tableop.KS,
}
NEW_KS = {
    "lookup, histogram": CHEAP_KS,
    "text_counts": CHEAP_KS,
    "seq_stats": CHEAP_KS,
    "compact": CHEAP_KS,
    "count": CHEAP_KS,
    "correct": HEAVY_NEW_KS,
    "neighbors, graph": HEAVY_NEW_KS,
    "unitigs": HEAVY_NEW_KS,
    "table_op": HEAVY_NEW_KS,
}


def width_input(k, other=0):
    """the FASTA bytes of the width tests at k: test_gpu_graph's reads up to three-word keys (100-base
    reads), test_gpu_unitig's 600-base reads from 95 on (make_reads(95) has only 70 unitigs of at
    most 10 nodes from T(c) >= 2 on); other: added to the seed, for reads of another genome"""
    if k <= 65:
        return test_gpu_graph.make_reads(k + other)
    if k >= 95:
        return test_gpu_unitig.wide_reads(1000 + k + other)
    raise ValueError(f"no width input for k = {k}")
