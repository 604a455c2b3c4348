// kc_key.h -- arithmetic on a k-mer held as W 64-bit words (character 0, the leftmost, in the
// highest of the 2k bits; word 0 the most significant): reading and setting a character, shifting
// one in at either end, comparing, and the eight de Bruijn neighbours of a k-mer.  Shared by the
// compaction (kc_compact_impl.h), the graph (kc_graph_impl.h) and the unitigs (kc_unitig_impl.h).
#pragma once
#include "kc_common.h"

namespace kc {

template <int W>
DEV uint32_t key_char(const uint64_t (&K)[W], int k, int j) {  // character j (0 = leftmost)
    const int pos = 2 * (k - 1 - j);
    const int wi = W - 1 - (pos >> 6);
    uint64_t w = 0;
#pragma unroll
    for (int i = 0; i < W; i++)
        if (i == wi) w = K[i];
    return (uint32_t)(w >> (pos & 63)) & 3;
}
template <int W>
DEV void or_char(uint64_t (&K)[W], int k, int j, uint32_t c) {
    const int pos = 2 * (k - 1 - j);
    const int wi = W - 1 - (pos >> 6);
#pragma unroll
    for (int i = 0; i < W; i++)
        if (i == wi) K[i] |= (uint64_t)c << (pos & 63);
}
// P = c followed by the first k - 1 characters of X
template <int W>
DEV void prepend_char(const uint64_t (&X)[W], uint32_t c, const RollConst& rk, uint64_t (&P)[W]) {
#pragma unroll
    for (int i = W - 1; i >= 1; i--) P[i] = (X[i] >> 2) | (X[i - 1] << 62);
    P[0] = X[0] >> 2;
#pragma unroll
    for (int i = 0; i < W; i++)
        if (i == rk.rc_word) P[i] |= (uint64_t)c << rk.rc_bit;
}
// P = X[1:] + c: X shifted left one character, c appended
template <int W>
DEV void append_char(const uint64_t (&X)[W], uint32_t c, const RollConst& rk, uint64_t (&P)[W]) {
#pragma unroll
    for (int i = 0; i < W - 1; i++) P[i] = (X[i] << 2) | (X[i + 1] >> 62);
    P[W - 1] = (X[W - 1] << 2) | c;
    P[0] &= rk.topmask;
}
template <int W>
DEV bool key_le(const uint64_t (&a)[W], const uint64_t (&b)[W]) {
#pragma unroll
    for (int i = 0; i < W; i++)
        if (a[i] != b[i]) return a[i] < b[i];
    return true;
}
template <int W>
DEV bool key_eq(const uint64_t (&a)[W], const uint64_t (&b)[W]) {
    bool eq = true;
#pragma unroll
    for (int i = 0; i < W; i++) eq &= a[i] == b[i];
    return eq;
}

// Neighbour i of the k-mer K (RC its reverse complement): i = y on side R, z = K[1:] + y, and
// i = 4 + y on side L, z = y + K[:-1].  rc(z) comes from RC by the opposite shift with 3 - y, so no
// neighbour is reverse-complemented on its own.  t = the table key of canon(z).  Returns 0 when z
// is the canonical form (z < rc(z)), 1 when rc(z) is, 2 when z is its own reverse complement.
template <int W>
DEV int neighbor_tkeys(const uint64_t (&K)[W], const uint64_t (&RC)[W], int i, const RollConst& rk, uint64_t (&t)[W]) {
    const uint32_t y = (uint32_t)i & 3;
    uint64_t z[W], rz[W];
    if (i < 4) {
        append_char<W>(K, y, rk, z);
        prepend_char<W>(RC, 3 - y, rk, rz);
    } else {
        prepend_char<W>(K, y, rk, z);
        append_char<W>(RC, 3 - y, rk, rz);
    }
    const bool le = key_le<W>(z, rz), ge = key_le<W>(rz, z);
    uint64_t d[W];
#pragma unroll
    for (int j = 0; j < W; j++) d[j] = le ? z[j] : rz[j];
    to_tkey<W>(d, t);
    return le ? (ge ? 2 : 0) : 1;
}

}  // namespace kc
