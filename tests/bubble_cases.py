"""Hand-built inputs of the bubble-popping tests (test_bubble_model.py on the CPU, test_gpu_bubble.py
and test_gpu_bubble_cli.py on the GPU), beside clean_cases.py: lists of sequences (str) whose k-mers
make a graph with a known shape.  All are random over ACGT from a seeded generator; every test still
asserts the shape on the model first.

A variant of genome g at position q is a copy of g[q - k : q + k + 1] -- 2 k + 1 bases, q in the
middle -- with base q changed: its first and last k-mers are the genome's, and the k between them (k -
1 when the base is deleted) are new nodes that run beside the genome's k nodes over q, between the
same two junctions."""
import numpy as np

from clean_cases import BASES, rand

KINDS = ("sub", "sub2", "del", "sub")


def substituted(g, q, k, step):
    return g[q - k:q] + BASES[(BASES.index(g[q]) + step) % 4] + g[q + 1:q + k + 1]


def variants(k, seed=21, sites=4, heavy=3):
    """a random genome of (sites + 1) * 3 k nodes given `heavy` times and, once each, a variant at q =
    (i + 1) * 3 k for site i: a substitution; two different substitutions (three arms); one base
    deleted; a substitution; and so on in turn.  (sequences, [(site, kind, variant)])"""
    rng = np.random.default_rng(seed)
    g = rand(rng, (sites + 1) * 3 * k + k - 1)
    for i in range(sites):
        if KINDS[i % 4] == "del":
            # a base that differs from both its neighbours: deleted from a run of r equal bases it
            # would leave k - r new nodes, not k - 1
            q = (i + 1) * 3 * k
            g = g[:q] + next(b for b in BASES if b not in (g[q - 1], g[q + 1])) + g[q + 1:]
    alts = []
    for i in range(sites):
        q = (i + 1) * 3 * k
        kind = KINDS[i % 4]
        if kind == "del":
            alts.append((i, kind, g[q - k:q] + g[q + 1:q + k + 1]))
        else:
            alts.append((i, kind, substituted(g, q, k, 1)))
            if kind == "sub2":
                alts.append((i, kind, substituted(g, q, k, 2)))
    return [g] * heavy + [a for _, _, a in alts], alts


def dense(k, seed, length=400, sites=40):
    """many substitutions on a short genome at a small k: accidental repeats and, at even k,
    palindromic nodes beside the bubbles.  The genome twice and one variant per site."""
    rng = np.random.default_rng(seed)
    g = rand(rng, length)
    seqs = [g, g]
    for q in rng.integers(k, length - k - 1, sites).tolist():
        seqs.append(substituted(g, q, k, int(rng.integers(1, 4))))
    return seqs


def palindromic_anchor(k, seed=31, tail=20):
    """even k: a palindromic k-mer P, then a base that differs between the two sequences, then a common
    tail -- two arms of k nodes that leave the one-node palindromic unitig P and meet again.  The first
    sequence is given twice.  (sequences, P)"""
    assert k % 2 == 0
    rng = np.random.default_rng(seed)
    h = rand(rng, k // 2)
    p = h + h[::-1].translate(str.maketrans("ACGT", "TGCA"))
    rest = rand(rng, k - 1 + tail)
    a, b = "AC" if rest[0] in "GT" else "GT"
    return [p + a + rest] * 2 + [p + b + rest], p
