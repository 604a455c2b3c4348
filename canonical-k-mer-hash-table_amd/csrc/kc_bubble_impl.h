// kc_bubble_impl.h -- bubble popping (include/kc_api.h kc_pop_bubbles_device): the two kernels that
// give every unitig of the range's graph its verdict, for one key width W (instantiated by
// kc_bubble_w.hip).  Before them on the stream: the ranking and k_unitig_heads (start[id] of every
// node); after them k_clean (kc_clean_impl.h), which copies the nodes of every unitig whose verdict
// is CLEAN_KEEP.
//
//   k_bubble_anchors  over the node ids.  The node at position 0 of its unitig (found as
//                     k_unitig_verdict finds it) has the unitig's two end states.  An open unitig
//                     whose ends both have degree 1 rebuilds each end node's k-mer from its slot,
//                     forms the one neighbour's table key and probes once for its slot; the anchor
//                     is 2 * the neighbour's node id + the facing side (R for a palindromic
//                     neighbour: its side-R nibble holds all its neighbours).  anc[2 start + e] =
//                     the anchor of end e, or UNITIG_NO_ID at both when the unitig is no branch: a
//                     palindromic node, an edge into itself, two equal anchors, or any value that
//                     cannot be followed.  The launcher fills anc with UNITIG_NO_ID first, so every
//                     id that starts no branch reads so.
//   k_bubble_verdict  over the node ids again.  A branch (anc[2 i] set) walks the at most four set
//                     bits of the edge nibble of its first anchor end, probes each neighbour once
//                     and follows slot -> id -> start; a start S other than its own whose two anchors
//                     are, as a set, its own is a parallel branch.  n and count_sum of S are read
//                     from the two final states at id S and tc[S], as its own are.  The rule of
//                     include/kc_api.h decides; the end nodes' keys, for the name, are loaded only
//                     when the two products are equal.  CLEAN_BUBBLE at verdict[i] pops it.
//
// The table is only read (kc_table_read.h: plain loads, every probe bounded by BPR).  Every index
// followed is bounded first: an id and a start below the node count, a state below twice that, a
// slot below the slot count.  Statistics are reduced per workgroup (kc_block.h).
#pragma once
#include "kc_unit_read.h"

namespace kc {

constexpr int BUBBLE_T = BLOCK_T;
constexpr uint64_t BUBBLE_BLOCKS = 8192;  // grid-stride: 32 workgroups per CU

struct BubbleArgs {
    TableView tv;
    int k, j;                   // j: the control word of the ranking's final buffer (UC_SRC + j)
    UnitigBufs u;
    uint32_t* anc;              // [2 start id + e]
    BubbleRule rule;
    unsigned long long* stats;  // kc_bubble_stats as eight words (nullptr: none)
};

// (bubble_unit and bubble_node_key: kc_unit_read.h, shared with kc_weak_impl.h)

// the anchor of the unitig end at state x of the unitig that starts at `own`: UNITIG_NO_ID when the
// end's node is palindromic, its degree is not 1, or its neighbour is not found or starts at `own`
template <int W>
DEV uint32_t bubble_anchor(const BubbleArgs& g, const RollConst& rk, uint32_t x, uint32_t own, uint64_t n_nodes,
                           uint64_t n_slots) {
    uint64_t slot, K[W], RC[W], t[W];
    if (!bubble_node_key<W>(g.tv, g.u, x >> 1, n_slots, slot, K)) return UNITIG_NO_ID;
    revcomp<W>(K, rk, RC);
    if (key_eq<W>(K, RC)) return UNITIG_NO_ID;
    const int side = (int)(x & 1);
    const uint32_t nib = ((uint32_t)g.u.edges[slot] >> (4 * side)) & 15;
    if (__popc(nib) != 1) return UNITIG_NO_ID;
    const int ori = neighbor_tkeys<W>(K, RC, 4 * side + (__ffs((int)nib) - 1), rk, t);
    const uint32_t facing = ori == 2 ? 0u : ((ori == 0) == (side == 0) ? 1u : 0u);
    const uint64_t ds = graph_probe_slot<W>(g.tv, t);
    if (ds == NO_SLOT || ds >= n_slots) return UNITIG_NO_ID;
    const uint32_t did = g.u.id_of_slot[ds];
    if (did >= n_nodes) return UNITIG_NO_ID;
    const uint32_t sd = g.u.start[did];
    if (sd >= n_nodes || sd == own) return UNITIG_NO_ID;
    return 2 * did + facing;
}

template <int W>
__global__ __launch_bounds__(BUBBLE_T) void k_bubble_anchors(BubbleArgs g) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    const RollConst rk = make_roll<W>(g.k, 0, 0);
    const uint64_t n_nodes = unitig_nodes(g.u), n_states = 2 * n_nodes, n_slots = g.tv.nbuckets * S;
    const UnitigState* __restrict__ F = g.u.st[g.u.ctl[UC_SRC + g.j] & 1];
    unsigned long long n_unitigs = 0, n_mine = 0, n_branches = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * BUBBLE_T + threadIdx.x; i < n_nodes; i += (uint64_t)gridDim.x * BUBBLE_T) {
        n_mine++;
        const BubbleUnit un = bubble_unit(g.u, F, i, n_states);
        if (!un.head) continue;
        n_unitigs++;
        uint32_t a0 = UNITIG_NO_ID, a1 = UNITIG_NO_ID;
        if (g.u.succ[un.a] == UNITIG_END && g.u.succ[un.b] == UNITIG_END &&  // open
            unitig_end_degree(g.u, un.a, n_slots) == 1 && unitig_end_degree(g.u, un.b, n_slots) == 1) {
            a0 = bubble_anchor<W>(g, rk, un.a, (uint32_t)i, n_nodes, n_slots);
            if (a0 != UNITIG_NO_ID) a1 = bubble_anchor<W>(g, rk, un.b, (uint32_t)i, n_nodes, n_slots);
            if (a1 == UNITIG_NO_ID || a1 == a0) a0 = a1 = UNITIG_NO_ID;
        }
        g.anc[2 * i] = a0;
        g.anc[2 * i + 1] = a1;
        n_branches += a0 != UNITIG_NO_ID;
    }
    const unsigned long long v[3] = {n_unitigs, n_mine, n_branches};
    unsigned long long* const st = g.stats;
    unsigned long long* const dst[3] = {st, st ? st + 1 : nullptr, st ? st + 2 : nullptr};
    block_sum_add<3>(v, dst);
}

// name(U) of the unitig with the end states a and b: the smaller of its two end nodes' canonical
// k-mers (the key words compare as the strings do); false: a slot cannot be followed
template <int W>
DEV bool bubble_name(const BubbleArgs& g, uint32_t a, uint32_t b, uint64_t n_slots, uint64_t (&N)[W]) {
    uint64_t slot, X[W];
    if (!bubble_node_key<W>(g.tv, g.u, a >> 1, n_slots, slot, N)) return false;
    if ((b >> 1) == (a >> 1)) return true;
    if (!bubble_node_key<W>(g.tv, g.u, b >> 1, n_slots, slot, X)) return false;
    if (!key_le<W>(N, X)) {
#pragma unroll
        for (int j = 0; j < W; j++) N[j] = X[j];
    }
    return true;
}

// x * y as (hi, lo)
DEV void bubble_mul(uint64_t x, uint64_t y, uint64_t& hi, uint64_t& lo) {
    hi = __umul64hi(x, y);
    lo = x * y;
}

template <int W>
__global__ __launch_bounds__(BUBBLE_T) void k_bubble_verdict(BubbleArgs g) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    const RollConst rk = make_roll<W>(g.k, 0, 0);
    const uint64_t n_nodes = unitig_nodes(g.u), n_states = 2 * n_nodes, n_slots = g.tv.nbuckets * S;
    const UnitigState* __restrict__ F = g.u.st[g.u.ctl[UC_SRC + g.j] & 1];
    const BubbleRule rule = g.rule;
    unsigned long long n_par = 0, n_pop = 0, n_pop_nodes = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * BUBBLE_T + threadIdx.x; i < n_nodes; i += (uint64_t)gridDim.x * BUBBLE_T) {
        const uint32_t A = g.anc[2 * i], B = g.anc[2 * i + 1];
        if (A == UNITIG_NO_ID || B == UNITIG_NO_ID || (A >> 1) >= n_nodes) continue;  // no branch starts here
        const BubbleUnit me = bubble_unit(g.u, F, i, n_states);
        const bool can_go = rule.max_nodes && me.n <= rule.max_nodes &&
                            (!rule.max_mean || me.sum <= (uint64_t)rule.max_mean * me.n);
        uint64_t slot, K[W], RC[W];
        if (!bubble_node_key<W>(g.tv, g.u, A >> 1, n_slots, slot, K)) continue;
        revcomp<W>(K, rk, RC);
        const int side = (int)(A & 1);
        uint32_t nib = ((uint32_t)g.u.edges[slot] >> (4 * side)) & 15;
        bool parallel = false, popped = false;
        // the parallel branches whose product equals mine (at most three): their names decide, after
        // the walk, when its keys are no longer held
        uint32_t tie0 = UNITIG_NO_ID, tie1 = UNITIG_NO_ID, tie2 = UNITIG_NO_ID;
#pragma unroll 1
        for (; nib; nib &= nib - 1) {
            uint64_t t[W];
            neighbor_tkeys<W>(K, RC, 4 * side + (__ffs((int)nib) - 1), rk, t);
            const uint64_t ds = graph_probe_slot<W>(g.tv, t);
            if (ds == NO_SLOT || ds >= n_slots) continue;
            const uint32_t did = g.u.id_of_slot[ds];
            if (did >= n_nodes) continue;
            const uint32_t s2 = g.u.start[did];
            if (s2 >= n_nodes || s2 == i) continue;
            const uint32_t A2 = g.anc[2 * (uint64_t)s2], B2 = g.anc[2 * (uint64_t)s2 + 1];
            if (!((A2 == A && B2 == B) || (A2 == B && B2 == A))) continue;
            parallel = true;
            if (!can_go || popped) continue;
            const BubbleUnit it = bubble_unit(g.u, F, s2, n_states);
            const uint64_t diff = it.n > me.n ? it.n - me.n : me.n - it.n;
            if (it.n > rule.max_nodes || diff > rule.max_diff) continue;
            // it beats me: count_sum(it) * n(me) > count_sum(me) * n(it), or equal and the smaller name
            uint64_t h1, l1, h2, l2;
            bubble_mul(it.sum, me.n, h1, l1);
            bubble_mul(me.sum, it.n, h2, l2);
            if (h1 != h2 || l1 != l2) {
                popped = h1 != h2 ? h1 > h2 : l1 > l2;
            } else if (tie0 == UNITIG_NO_ID) {
                tie0 = s2;
            } else if (tie1 == UNITIG_NO_ID) {
                tie1 = s2;
            } else {
                tie2 = s2;
            }
        }
        if (!popped && tie0 != UNITIG_NO_ID) {
            uint64_t mine[W];
            if (bubble_name<W>(g, me.a, me.b, n_slots, mine)) {
#pragma unroll 1
                for (int q = 0; q < 3 && !popped; q++) {
                    const uint32_t s2 = q == 0 ? tie0 : q == 1 ? tie1 : tie2;
                    if (s2 == UNITIG_NO_ID) break;
                    const BubbleUnit it = bubble_unit(g.u, F, s2, n_states);
                    uint64_t its[W];
                    if (bubble_name<W>(g, it.a, it.b, n_slots, its)) popped = !key_le<W>(mine, its);
                }
            }
        }
        n_par += parallel;
        if (popped) {
            g.u.verdict[i] = CLEAN_BUBBLE;
            n_pop++;
            n_pop_nodes += me.n;
        }
    }
    const unsigned long long v[3] = {n_par, n_pop, n_pop_nodes};
    unsigned long long* const st = g.stats;
    unsigned long long* const dst[3] = {st ? st + 3 : nullptr, st ? st + 4 : nullptr, st ? st + 5 : nullptr};
    block_sum_add<3>(v, dst);
}

template <int W>
hipError_t BubbleOps<W>::pop(TableView src, int k, UnitigBufs u, int rounds, uint32_t* anc, BubbleRule rule,
                             unsigned long long* stats, hipStream_t s) {
    if (!u.verdict || !anc) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(u.verdict, CLEAN_KEEP, u.bound, s);
    if (e != hipSuccess) return e;
    if (!src.nbuckets) return hipSuccess;
    if ((e = hipMemsetAsync(anc, 0xFF, 2 * u.bound * sizeof(uint32_t), s)) != hipSuccess) return e;
    const BubbleArgs g{src, k, 2 * rounds, u, anc, rule, stats};
    const uint64_t need = (u.bound + BUBBLE_T - 1) / BUBBLE_T;
    const unsigned grid = (unsigned)(need < BUBBLE_BLOCKS ? (need ? need : 1) : BUBBLE_BLOCKS);
    hipLaunchKernelGGL(k_bubble_anchors<W>, dim3(grid), dim3(BUBBLE_T), 0, s, g);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_bubble_verdict<W>, dim3(grid), dim3(BUBBLE_T), 0, s, g);
    return hipGetLastError();
}

}  // namespace kc
