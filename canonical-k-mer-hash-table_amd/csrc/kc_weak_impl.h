// kc_weak_impl.h -- weak-link removal (include/kc_api.h kc_cut_weak_device): the kernel that gives
// every unitig of the range's graph its verdict, for one key width W (instantiated by
// kc_weak_w.hip).  Before it on the stream: the ranking and k_unitig_heads (start[id] of every
// node); after it k_clean (kc_clean_impl.h), which copies the nodes of every unitig whose verdict is
// CLEAN_KEEP.
//
//   k_weak_verdict  over the node ids.  The node at position 0 of its unitig (found as
//                   k_bubble_anchors finds it) has the unitig's two end states.  An open unitig whose
//                   ends both have an edge rebuilds each end node's k-mer from its slot -- a node that
//                   is its own reverse complement makes the unitig palindromic, not interior -- and
//                   walks the set bits of the end's edge nibble: the neighbour's table key, one
//                   probe for its slot, slot -> id -> start.  A start other than its own is one
//                   entry of N(U): n and count_sum of that unitig are read from the two final
//                   states at its start id and tc[], as its own are, and added to local_n and
//                   local_sum.  The rule of include/kc_api.h decides, its two products as (hi, lo)
//                   pairs (kc_weak_rule.h); CLEAN_WEAK at verdict[i] cuts it.  An interior unitig
//                   costs at most eight probes.
//
// The table is only read (kc_table_read.h: plain loads, every probe bounded by BPR).  Every index
// followed is bounded first: an id and a start below the node count, a state below twice that, a
// slot below the slot count.  Statistics are reduced per workgroup (kc_block.h).
#pragma once
#include "kc_unit_read.h"
#include "kc_weak_rule.h"

namespace kc {

constexpr int WEAK_T = BLOCK_T;
constexpr uint64_t WEAK_BLOCKS = 8192;  // grid-stride: 32 workgroups per CU

struct WeakArgs {
    TableView tv;
    int k, j;                   // j: the control word of the ranking's final buffer (UC_SRC + j)
    UnitigBufs u;
    WeakRule rule;
    unsigned long long* stats;  // kc_weak_stats as eight words (nullptr: none); this kernel's are 0 to 5
};

// N(U) over the edges of the unitig end at state x of the unitig that starts at `own`: n and
// count_sum of every neighbour's unitig other than `own` added to loc.  false: the end's node is
// its own reverse complement (U is palindromic) or its slot cannot be followed
template <int W>
DEV bool weak_end(const WeakArgs& g, const RollConst& rk, const UnitigState* __restrict__ F, uint32_t x, uint32_t own,
                  uint64_t n_nodes, uint64_t n_slots, WeakLocal& loc) {
    uint64_t slot, K[W], RC[W];
    if (!bubble_node_key<W>(g.tv, g.u, x >> 1, n_slots, slot, K)) return false;
    revcomp<W>(K, rk, RC);
    if (key_eq<W>(K, RC)) return false;
    const int side = (int)(x & 1);
    uint32_t nib = ((uint32_t)g.u.edges[slot] >> (4 * side)) & 15;
#pragma unroll 1
    for (; nib; nib &= nib - 1) {
        uint64_t t[W];
        neighbor_tkeys<W>(K, RC, 4 * side + (__ffs((int)nib) - 1), rk, t);
        const uint64_t ds = graph_probe_slot<W>(g.tv, t);
        if (ds == NO_SLOT || ds >= n_slots) continue;
        const uint32_t did = g.u.id_of_slot[ds];
        if (did >= n_nodes) continue;
        const uint32_t s2 = g.u.start[did];
        if (s2 >= n_nodes || s2 == own) continue;  // an edge back into U gives no entry
        const BubbleUnit it = bubble_unit(g.u, F, s2, 2 * n_nodes);
        weak_local_add(loc, it.n, it.sum);
    }
    return true;
}

template <int W>
__global__ __launch_bounds__(WEAK_T) void k_weak_verdict(WeakArgs g) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    const RollConst rk = make_roll<W>(g.k, 0, 0);
    const uint64_t n_nodes = unitig_nodes(g.u), n_states = 2 * n_nodes, n_slots = g.tv.nbuckets * S;
    const UnitigState* __restrict__ F = g.u.st[g.u.ctl[UC_SRC + g.j] & 1];
    const WeakRule rule = g.rule;
    unsigned long long n_unitigs = 0, n_mine = 0, n_interior = 0, n_weak = 0, n_cut = 0, n_cut_nodes = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * WEAK_T + threadIdx.x; i < n_nodes; i += (uint64_t)gridDim.x * WEAK_T) {
        n_mine++;
        const BubbleUnit me = bubble_unit(g.u, F, i, n_states);
        if (!me.head) continue;
        n_unitigs++;
        if (g.u.succ[me.a] != UNITIG_END || g.u.succ[me.b] != UNITIG_END) continue;  // circular
        if (!unitig_end_degree(g.u, me.a, n_slots) || !unitig_end_degree(g.u, me.b, n_slots)) continue;
        WeakLocal loc{0, 0, 0};
        bool interior = true;
#pragma unroll 1
        for (int e = 0; e < 2 && interior; e++)
            interior = weak_end<W>(g, rk, F, e ? me.b : me.a, (uint32_t)i, n_nodes, n_slots, loc);
        if (!interior) continue;
        n_interior++;
        if (!loc.n || (rule.ratio_permille && !weak_below(me.sum, me.n, loc, rule.ratio_permille))) continue;
        n_weak++;
        if (rule.max_nodes && me.n <= rule.max_nodes && (!rule.max_mean || me.sum <= (uint64_t)rule.max_mean * me.n)) {
            g.u.verdict[i] = CLEAN_WEAK;
            n_cut++;
            n_cut_nodes += me.n;
        }
    }
    const unsigned long long v[6] = {n_unitigs, n_mine, n_interior, n_weak, n_cut, n_cut_nodes};
    unsigned long long* const st = g.stats;
    unsigned long long* const dst[6] = {st,
                                        st ? st + 1 : nullptr,
                                        st ? st + 2 : nullptr,
                                        st ? st + 3 : nullptr,
                                        st ? st + 4 : nullptr,
                                        st ? st + 5 : nullptr};
    block_sum_add<6>(v, dst);
}

template <int W>
hipError_t WeakOps<W>::cut(TableView src, int k, UnitigBufs u, int rounds, WeakRule rule, unsigned long long* stats,
                           hipStream_t s) {
    if (!u.verdict) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(u.verdict, CLEAN_KEEP, u.bound, s);
    if (e != hipSuccess || !src.nbuckets) return e;
    const WeakArgs g{src, k, 2 * rounds, u, rule, stats};
    const uint64_t need = (u.bound + WEAK_T - 1) / WEAK_T;
    const unsigned grid = (unsigned)(need < WEAK_BLOCKS ? (need ? need : 1) : WEAK_BLOCKS);
    hipLaunchKernelGGL(k_weak_verdict<W>, dim3(grid), dim3(WEAK_T), 0, s, g);
    return hipGetLastError();
}

}  // namespace kc
