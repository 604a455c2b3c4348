// kc_unit_read.h -- what the verdict kernels of bubble popping (kc_bubble_impl.h) and of weak-link
// removal (kc_weak_impl.h) both read of the ranked graph, after k_unitig_heads: the unitig a node
// belongs to from its two final states, and a node's canonical k-mer from its slot.  Every index
// followed is bounded first.
#pragma once
#include "kc_graph_impl.h"

namespace kc {

// the unitig that node i belongs to as its two final states tell it (as k_unitig_heads reads them; a
// state that is not DONE stands alone): the end states through R and L, n and count_sum, and
// whether i is the node at position 0
struct BubbleUnit {
    uint32_t a, b;
    uint64_t n, sum;
    bool head;
};
DEV BubbleUnit bubble_unit(const UnitigBufs& u, const UnitigState* __restrict__ F, uint64_t i, uint64_t n_states) {
    const UnitigState r = F[2 * i], l = F[2 * i + 1];
    uint32_t a = r.nxt & ~UNITIG_DONE, b = l.nxt & ~UNITIG_DONE, dR = r.dist, dL = l.dist;
    uint64_t sR = r.sum, sL = l.sum;
    if (!(r.nxt & UNITIG_DONE) || a >= n_states) a = (uint32_t)(2 * i), dR = 0, sR = 0;
    if (!(l.nxt & UNITIG_DONE) || b >= n_states) b = (uint32_t)(2 * i + 1), dL = 0, sL = 0;
    const bool fwd = (b >> 1) <= (a >> 1);
    return BubbleUnit{a, b, (uint64_t)dR + dL + 1, sR + sL + u.tc[i], (fwd ? dL : dR) == 0};
}

// the canonical k-mer of node id (< the node count) into K; false: its slot cannot be followed
template <int W>
DEV bool bubble_node_key(const TableView& tv, const UnitigBufs& u, uint32_t id, uint64_t n_slots, uint64_t& slot,
                         uint64_t (&K)[W]) {
    slot = u.slot_of[id];
    if (slot >= n_slots) return false;
    uint64_t tk[W];
    slot_tkey<W>(tv, slot, tk);
    if (tk[0] == EMPTY) return false;
    from_tkey<W>(tk, K);
    return true;
}

}  // namespace kc
