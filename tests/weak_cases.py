"""Hand-built inputs of the weak-link tests (test_weak_model.py on the CPU, test_gpu_weak.py and
test_gpu_weak_cli.py on the GPU), beside clean_cases.py and bubble_cases.py: lists of sequences (str)
whose k-mers make a graph with a known shape.  All are random over ACGT from a seeded generator; every
test still asserts the shape on the model first.

A joint of G1 at a and G2 at b is G1[a - k + 1 : a] + G2[b : b + k - 1]: 2 k - 2 bases whose k - 1
k-mers each hold bases of both -- no k-mer of G1 or G2 -- and that run from G1's node a - k to G2's
node b: one unitig connected at both ends, which cuts each of G1 and G2 into two unitigs."""
import numpy as np

from clean_cases import BASES, rand

import graph_model as m

# what test_gpu_clean and test_gpu_unitig give as a FASTA text: poly-A (one node whose two ends lead
# into itself), a two-node circle and a hairpin (a read that runs on into its own reverse complement)
HAIR = "ACGGTCAATGCCTGAAGTCCATGACCGTTAGACT"
SELF_LOOPS = ["A" * 60, "CA" * 40, HAIR + m.rc(HAIR)]


def other(base, step=1):
    return BASES[(BASES.index(base) + step) % 4]


def joint(g1, a, g2, b, k):
    """the joint of g1 at a and g2 at b; its first k-mer must not be g1's next and its last not g2's"""
    assert g2[b] != g1[a] and g1[a - 1] != g2[b - 1]
    return g1[a - k + 1:a] + g2[b:b + k - 1]


def two_genomes(k, seed, nodes=100):
    """two random sequences of `nodes` nodes each and the places a, b of a joint in their middles"""
    rng = np.random.default_rng(seed)
    g1, g2 = rand(rng, nodes + k - 1), rand(rng, nodes + k - 1)
    a, b = nodes // 2 + k - 1, nodes // 2  # G1 is left after its node nodes / 2 - 1, G2 entered at its node nodes / 2
    # the base after the joint differs from G1's own, the base before it from G2's own
    g2 = g2[:b - 1] + other(g1[a - 1]) + other(g1[a]) + g2[b + 1:]
    return g1, g2, a, b


def chimera(k, seed=41, heavy=10, light=1):
    """G1 and G2 `heavy` times each and the joint of their middles `light` times: (sequences, the joint)"""
    g1, g2, a, b = two_genomes(k, seed)
    j = joint(g1, a, g2, b, k)
    return [g1] * heavy + [g2] * heavy + [j] * light, j


def het_bubble(k, seed=42, each=5):
    """an even heterozygous site: a genome of 100 nodes and its copy with the middle base substituted,
    `each` times each -- two arms of k nodes and mean `each` between flanks of mean 2 * each"""
    rng = np.random.default_rng(seed)
    g = rand(rng, 100 + k - 1)
    q = 50 + k - 1
    alt = g[:q] + other(g[q]) + g[q + 1:]
    return [g] * each + [alt] * each, q


def double_neighbour(k, seed=43, heavy=10, bridge=2, n_v=50, n_w=50, mid=5):
    """a genome Y V X `heavy` times; a bridge from V's end back to V's start, `bridge` times: the last
    k - 1 bases of V, `mid` bases, the first k - 1 bases of V -- mid + k - 1 nodes whose two ends both
    hang on V; and once a branch W of n_w nodes off V's first k - 1 bases, which the bridge's end
    reaches too.  N(bridge) = {V, V, W}.  (sequences, the bridge, V, W's sequence)"""
    rng = np.random.default_rng(seed)
    y, v, x = rand(rng, 40), rand(rng, n_v + k - 1), rand(rng, 40)
    m_ = rand(rng, mid)
    m_ = other(x[0]) + m_[1:-1] + other(y[-1])  # it leaves V beside X and comes back beside Y
    b = v[-(k - 1):] + m_ + v[:k - 1]
    w = v[:k - 1] + other(v[k - 1]) + rand(rng, n_w - 1)
    return [y + v + x] * heavy + [b] * bridge + [w], b, v, w


def loop_end(k, seed=44, copies=10, tail=60):
    """k A's and a random tail, `copies` times, and k - 1 A's and the tail as often again: the node
    A^k has count `copies`, a self loop on either side and one more edge, to the tail's unitig of mean
    2 * copies.  Its left end's only edge leads back into it.  (sequences, the tail)"""
    rng = np.random.default_rng(seed)
    t = "C" + rand(rng, tail - 1)
    return ["A" * k + t] * copies + ["A" * (k - 1) + t] * copies, t


def palindrome(k, seed=45, flank=20, heavy=5):
    """even k: L1 X P Y once, with P a palindromic k-mer, and L1 X P[:-1] and P[1:] Y `heavy` times: P
    has count 1 between flanks of count heavy + 1.  A second way into X, L2, heavy + 1 times, and its
    first three nodes once more: the `flank` nodes of X before P are an interior unitig of mean
    heavy + 1 with N = {L1, L2, P}, whose mean is above heavy + 1 without P and below it with P.
    (sequences, P, X's unitig)"""
    assert k % 2 == 0 and flank > 3
    rng = np.random.default_rng(seed)
    h = rand(rng, k // 2)
    p = h + h[::-1].translate(str.maketrans("ACGT", "TGCA"))
    x, y, l1, l2 = rand(rng, flank), rand(rng, flank), rand(rng, flank), rand(rng, flank)
    l2 = l2[:-1] + other(l1[-1])
    into_x = l2 + (x + p)[:k - 1]
    seqs = [l1 + x + p + y] + [l1 + x + p[:-1]] * heavy + [p[1:] + y] * heavy + [into_x] * (heavy + 1) + [into_x[:k + 2]]
    return seqs, p, (x + p)[:flank + k - 1]


def big_counts(k=31, seed=46):
    """the chimera with every count times F in a -m 0 table (where T(c) = c mod 65536 is largest): the
    genomes' k-mers at 10 F and the joint's at F.  T(c) is below 2^16 in every mode, so the rule's two
    products pass 2^64 only when n(U) * local_n passes 2.8e11 -- no graph a test can hold -- but both
    are far above 2^32, and F is the largest for which products cut to 32 bits give the other verdict
    at RATIO (the joint's k - 1 nodes between 50 nodes of G1 and 50 of G2).  (sequences, the joint, F,
    RATIO)"""
    seqs, j = chimera(k, seed)
    ratio, n_u, local_n = 200, k - 1, 100
    for f in range(65535 // 10, 0, -1):
        lhs, rhs = f * n_u * local_n * 1000, ratio * 10 * f * local_n * n_u
        if lhs >= 1 << 32 and (lhs < rhs) != (lhs & 0xFFFFFFFF < rhs & 0xFFFFFFFF):
            return seqs, j, f, ratio
    raise AssertionError("no such factor")


def fasta(seqs):
    return "".join(f">s{i}\n{s}\n" for i, s in enumerate(seqs)).encode()
