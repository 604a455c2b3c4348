"""Hand-built inputs of the graph-cleaning tests (test_clean_model.py on the CPU, test_gpu_clean.py and
test_gpu_clean_cli.py on the GPU): lists of sequences (str) whose k-mers make a graph with a known
shape.  All are random over ACGT from a seeded generator, so at the k the tests use (15 and up) no
(k - 1)-mer repeats by accident; every test still asserts the shape on the model first.

A branch off sequence G at p is G[p : p + k - 1] plus t random bases, the first differing from
G[p + k - 1]: t new nodes that leave G's node p - 1 beside G's node p and end in a dead end."""
import numpy as np

BASES = "ACGT"


def rand(rng, n):
    return "".join(BASES[i] for i in rng.integers(0, 4, n))


def branch(rng, g, p, t, k):
    """the branch sequence of t nodes off g at p (0 < p, p + k - 1 < len(g))"""
    assert 0 < p and p + k - 1 < len(g) and t >= 1
    first = BASES[(BASES.index(g[p + k - 1]) + int(rng.integers(1, 4))) % 4]
    return g[p:p + k - 1] + first + rand(rng, t - 1)


def chain_with_branch(k, seed=1, t=3, heavy=1):
    """a genome of 40 + 50 nodes and one branch of t nodes off node 39, given `heavy` times:
    (sequences, the branch)"""
    rng = np.random.default_rng(seed)
    g = rand(rng, 90 + k - 1)
    b = branch(rng, g, 40, t, k)
    return [g] + [b] * heavy, b


def isolated_chain(k, seed=2, n=5):
    """a genome of 60 nodes and, apart from it, a chain of n nodes: (sequences, the chain)"""
    rng = np.random.default_rng(seed)
    g, c = rand(rng, 60 + k - 1), rand(rng, n + k - 1)
    return [g, c], c


def small_circle(k, seed=3, n=5):
    """a circle of n nodes beside a genome of 60: (sequences, the circle's period)"""
    rng = np.random.default_rng(seed)
    g, c = rand(rng, 60 + k - 1), rand(rng, n)
    reps = (n + k - 1 + n - 1) // n + 1
    return [g, c * reps], c


def bubble(k, seed=14):
    """a genome of 100 nodes and a copy of its middle with base 50 + k - 1 substituted: two arms of k
    nodes between the same two junctions.  (sequences, the substituted position)"""
    rng = np.random.default_rng(seed)
    g = rand(rng, 100 + k - 1)
    q = 50 + k - 1
    alt = g[q - k + 1:q] + BASES[(BASES.index(g[q]) + 1) % 4] + g[q + 1:q + k]
    return [g, alt], q


def two_tip_junction(k, seed=5, t=3):
    """a stem of 50 nodes whose end forks into two tips of t nodes each: (sequences, stem)"""
    rng = np.random.default_rng(seed)
    stem = rand(rng, 50 + k - 1)
    a = rand(rng, t)
    b = BASES[(BASES.index(a[0]) + 1) % 4] + rand(rng, t - 1)
    return [stem + a, stem + b], stem


def cascade(k, seed=6, n=3):
    """a genome of 40 + 50 nodes, a branch B of 2 n nodes off its node 39 and a sub-branch of n nodes
    off B's node n - 1: B's near piece (n nodes, between the two junctions), its far piece (n nodes) and
    the sub-branch (n nodes).  Round 1 of tip_max_nodes = n removes the far piece and the sub-branch,
    round 2 the near piece, round 3 nothing.  (sequences, B, the sub-branch)"""
    rng = np.random.default_rng(seed)
    g = rand(rng, 90 + k - 1)
    b = branch(rng, g, 40, 2 * n, k)
    c = branch(rng, b, n, n, k)
    return [g, b, c], b, c


def fasta(seqs):
    return "".join(f">s{i}\n{s}\n" for i, s in enumerate(seqs)).encode()
