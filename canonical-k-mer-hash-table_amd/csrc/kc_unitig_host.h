// kc_unitig_host.h -- the host arithmetic of the unitig layer (kc_api_unitig.cpp, kc_cli.cpp): the
// rounds the ranking enqueues, the scratch a call needs and the FASTA header of a unitig.  Plain
// C++ without a device call, so a stand-alone program checks it under the sanitizers
// (tools/unitig_host_check.cpp).
#pragma once
#include <stdint.h>

#include <cstdio>

namespace kc {

// the node ids a call can number: a state 2 * id + side and the DONE bit share 32 bits
constexpr uint64_t UNITIG_MAX_BOUND = 1ULL << 30;
// bytes of scratch per table slot (the edge byte, the slot's id) and per node id that fits: T(c) 4,
// slot 8, two successors 8, two states in two buffers 96, start 4, position 4, offset and length 16
constexpr uint64_t UNITIG_SLOT_BYTES = 5, UNITIG_NODE_BYTES = 140;
// kc_unitig_graph* only: the record index of the unitig that starts at the node id
constexpr uint64_t UNITIG_REC_BYTES = 4;
// kc_clean* only: the verdict of the unitig that starts at the node id
constexpr uint64_t UNITIG_VERDICT_BYTES = 1;
// kc_pop_bubbles* only: the two anchors of the unitig that starts at the node id
constexpr uint64_t UNITIG_ANCHOR_BYTES = 8;

// jump launches of one ranking over up to `bound` nodes: ceil(log2(2 * bound)) + 1, round r covers
// paths of 2^(r + 1) states
inline int unitig_rounds(uint64_t bound) {
    const uint64_t states = 2 * (bound ? bound : 1);
    int lg = 0;
    while (lg < 63 && (1ULL << lg) < states) lg++;
    return lg + 1;
}

// What a ranking is asked for on top of the per-node arrays every call has: rec, the record index
// of the unitig that starts at the node id (kc_unitig_graph*); verdict, its verdict byte (kc_clean*,
// kc_pop_bubbles*); anchors, its two anchors (kc_pop_bubbles*).  The calls name theirs here, so that
// no call site spells out three booleans.
struct UnitigWants {
    bool rec = false, verdict = false, anchors = false;
};
constexpr UnitigWants UNITIG_PLAIN{}, UNITIG_GRAPH{true, false, false}, UNITIG_CLEAN{false, true, false},
    UNITIG_BUBBLE{false, true, true};

// the scratch of a call, control words aside; 0: it overflows 64 bits
inline uint64_t unitig_scratch_bytes(uint64_t table_slots, uint64_t bound, UnitigWants w = UNITIG_PLAIN) {
    const uint64_t node = UNITIG_NODE_BYTES + (w.rec ? UNITIG_REC_BYTES : 0) + (w.verdict ? UNITIG_VERDICT_BYTES : 0) +
                          (w.anchors ? UNITIG_ANCHOR_BYTES : 0);
    if (table_slots > ~0ULL / UNITIG_SLOT_BYTES || bound > ~0ULL / node) return 0;
    const uint64_t a = table_slots * UNITIG_SLOT_BYTES, b = bound * node;
    return a + b < a ? 0 : a + b;
}

// The per-node arrays in one block of 64-bit words, the widest first so that each is aligned:
// offsets in words of the two state buffers (6 words a node each), slot_of, off (2), succ (1), then
// the three 32-bit arrays tc, start and pos (half a word a node, rounded up) and, where wanted, the
// verdict bytes (an eighth of a word a node, rounded up) behind them and two 32-bit anchors a node
// (one word) behind those: every other offset is the same with or without (the record indices of
// UnitigWants::rec are a buffer of their own)
struct UnitigLayout {
    uint64_t st0, st1, slot_of, off, succ, tc, start, pos, verdict, anchors, words;
};
inline UnitigLayout unitig_layout(uint64_t bound, UnitigWants w = UNITIG_PLAIN) {
    const uint64_t half = (bound + 1) / 2;
    UnitigLayout l;
    l.st0 = 0;
    l.st1 = l.st0 + 6 * bound;
    l.slot_of = l.st1 + 6 * bound;
    l.off = l.slot_of + bound;
    l.succ = l.off + 2 * bound;
    l.tc = l.succ + bound;
    l.start = l.tc + half;
    l.pos = l.start + half;
    l.verdict = l.pos + half;
    l.anchors = l.verdict + (w.verdict ? (bound + 7) / 8 : 0);
    l.words = l.anchors + (w.anchors ? bound : 0);
    return l;
}

// ">i LN:i:<bases> KC:i:<count_sum> km:f:<count_sum / n_nodes, one decimal>[ circular]" into buf;
// the length written (without the terminator), as snprintf counts it
inline int unitig_fasta_header(char* buf, size_t size, uint64_t index, uint64_t n_nodes, uint64_t count_sum, int k,
                               bool circular) {
    const double km = n_nodes ? (double)count_sum / (double)n_nodes : 0.0;
    return std::snprintf(buf, size, ">%llu LN:i:%llu KC:i:%llu km:f:%.1f%s", (unsigned long long)index,
                         (unsigned long long)(n_nodes + (uint64_t)(k > 0 ? k - 1 : 0)), (unsigned long long)count_sum, km,
                         circular ? " circular" : "");
}

}  // namespace kc
