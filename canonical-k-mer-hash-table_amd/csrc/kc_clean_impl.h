// kc_clean_impl.h -- graph cleaning (include/kc_api.h kc_clean_device): k_clean copies the nodes of
// the kept unitigs of one counted table into another, for one key width W (instantiated by
// kc_clean_w.hip).  Before it on the stream: the ranking and k_unitig_heads (start[id] of every
// node) and k_unitig_verdict (kc_unitig.hip: the verdict byte at every unitig's start id).
//
// k_clean strides over the node ids a tile of CLEAN_T at a time.  A node reads its unitig's start
// and that start's verdict; a kept node reads its slot's table key and count word in src
// (kc_table_read.h: plain loads, src is only read) and adds the raw count -- the count word without
// its flag, not T(c) -- into dst with table_insert (kc_table_insert.h), as k_join adds its results:
// the keys of a full-key table do not depend on its geometry, so dst's own TableView places them
// whatever dst's size.  start, verdict and slot_of are coalesced reads by id; the slot's key and
// count are one scattered read of the node's own bucket, and the insert is the scattered write
// every insert is.  No key or record goes through HBM between the two tables.
//
// Every index followed is bounded: an id below the node count, a start below the node count, a slot
// below src's slot count; a slot that is empty (it cannot be on a table that is only read) is
// skipped, since an all-zero key must never reach table_insert.
//
// out_keys, out_sum and dst's counters are reduced per workgroup: one atomic per non-zero field per
// workgroup (kc_block.h), a few thousand per field on a C2-sized graph.
#pragma once
#include "kc_block.h"
#include "kc_table_insert.h"
#include "kc_table_read.h"

namespace kc {

constexpr int CLEAN_T = BLOCK_T;
constexpr uint64_t CLEAN_BLOCKS = 4096;  // grid-stride: 16 workgroups per CU

struct CleanArgs {
    TableView src, dst;         // read, destination (dst.buckets == nullptr: statistics only)
    UnitigBufs u;               // start, slot_of, verdict and the node count
    DevCounters* ctr;           // dst's counters (nullptr without dst)
    unsigned long long* stats;  // kc_clean_stats as eight words (nullptr: none); this kernel's are 6 and 7
};

template <int W>
__global__ __launch_bounds__(CLEAN_T) void k_clean(CleanArgs g) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    const uint64_t n_nodes = unitig_nodes(g.u), n_slots = g.src.nbuckets * S;
    // kept nodes, the sum of their raw counts, counts added to dst, failed inserts
    unsigned long long n_out = 0, sum_out = 0, added = 0, n_fail = 0;
    const uint64_t tiles = (n_nodes + CLEAN_T - 1) / CLEAN_T;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t i = tile * CLEAN_T + threadIdx.x;
        if (i >= n_nodes) continue;
        const uint32_t st = g.u.start[i];
        if (st >= n_nodes || g.u.verdict[st] != CLEAN_KEEP) continue;
        const uint64_t slot = g.u.slot_of[i];
        if (slot >= n_slots) continue;
        uint64_t tk[W];
        slot_tkey<W>(g.src, slot, tk);
        const uint64_t raw = slot_count_word<W>(g.src, slot) & CNT_MASK;
        if (tk[0] == EMPTY || !raw) continue;
        n_out++;
        sum_out += raw;
        if (g.dst.buckets) {
            if (table_insert<W>(g.dst, tk, raw)) added += raw;
            else n_fail++;
        }
    }
    const unsigned long long v[4] = {n_out, sum_out, added, n_fail};
    unsigned long long* const st = g.stats;
    unsigned long long* const dst[4] = {st ? st + 6 : nullptr, st ? st + 7 : nullptr,
                                        g.ctr ? &g.ctr->inserted : nullptr, g.ctr ? &g.ctr->overflow : nullptr};
    block_sum_add<4>(v, dst);
}

template <int W>
hipError_t CleanOps<W>::copy(TableView src, TableView dst, UnitigBufs u, DevCounters* ctr, unsigned long long* stats,
                             hipStream_t s) {
    if (!src.nbuckets || !u.verdict) return hipSuccess;
    const CleanArgs g{src, dst, u, ctr, stats};
    const uint64_t need = (u.bound + CLEAN_T - 1) / CLEAN_T;
    const unsigned grid = (unsigned)(need < CLEAN_BLOCKS ? (need ? need : 1) : CLEAN_BLOCKS);
    hipLaunchKernelGGL(k_clean<W>, dim3(grid), dim3(CLEAN_T), 0, s, g);
    return hipGetLastError();
}

}  // namespace kc
