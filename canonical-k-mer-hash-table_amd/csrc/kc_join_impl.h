// kc_join_impl.h -- table algebra: k_join relates two counted full-key tables in HBM, for one
// key width W (instantiated by kc_join_w.hip).  The reference has no counterpart: it counts one
// input into one table (kmer_hash_table.cpp:2207-2567) and its users join output files.
//
// k_join sweeps table X a bucket per thread (eight 16-byte loads, as k_route_table / k_histo) and,
// for every occupied slot whose T(c) lies in X's range, probes table Y with the slot's table key --
// the keys of a full-key table do not depend on its geometry (kc_common.h), so Y's own TableView
// finds it whatever Y's size -- applies the operation to the two raw counts and adds the result
// into dst with table_insert (kc_table_insert.h).  Sweep, probe and insert are one kernel: no key or
// record goes through HBM between the three tables.
//
//   first launch   X = a, Y = b: every operation.  r = op(ca, cb), cb = 0 when b does not hold the
//                  key inside its range.
//   second launch  X = b, Y = a (the UNION operations only): the keys of b that a does not hold
//                  inside its range, r = op(0, cb) = cb.
//
// X and Y are only read, by the rules of kc_table_read.h (plain loads; a probe ends at the first
// bucket with a free slot): the sweep loads buckets with load_bucket, the probe of Y is
// table_count_word.  dst is written
// by table_insert's CAS / atomic adds alone, so inserts of several launches and of other writers
// of dst on the same stream order add up.
//
// Statistics and dst's counters are reduced per workgroup: one atomic per non-zero field per
// workgroup; the grid is capped and strides over the buckets, so a C2-sized table (31 M buckets)
// issues a few thousand atomics per field, not 10^5.
#pragma once
#include "kc_block.h"
#include "kc_table_insert.h"
#include "kc_table_read.h"

namespace kc {

constexpr int JOIN_T = BLOCK_T;
constexpr uint64_t JOIN_BLOCKS = 4096;  // grid-stride: 16 workgroups per CU

// the operation on raw counts (cb = 0: b does not hold the key); 0 = no record
DEV uint64_t join_apply(int op, uint64_t ca, uint64_t cb) {
    switch (op) {
    case KC_OP_INTERSECT_MIN: return cb ? (ca < cb ? ca : cb) : 0;
    case KC_OP_INTERSECT_SUM: return cb ? ca + cb : 0;
    case KC_OP_INTERSECT_LEFT: return cb ? ca : 0;
    case KC_OP_SUBTRACT: return cb ? 0 : ca;
    case KC_OP_COUNTS_SUBTRACT: return ca > cb ? ca - cb : 0;
    case KC_OP_UNION_SUM: return ca + cb;
    default: return ca > cb ? ca : cb;  // KC_OP_UNION_MAX
    }
}

struct JoinArgs {
    TableView x, y, dst;        // swept, probed, destination (dst.buckets == nullptr: statistics only)
    int mode_x, mode_y;         // count modes of tc_of (0: -m 0, 1: -m 1/2)
    uint32_t x_min, x_max;      // x's range on T(c) (x_min >= 1, x_max 0 = no upper bound)
    uint32_t y_min, y_max;
    int op;
    int second;                 // the UNION operations' second launch (x = b, y = a)
    DevCounters* ctr;           // dst's counters (nullptr without dst)
    unsigned long long* stats;  // kc_op_stats as five words (nullptr: none)
};

template <int W>
__global__ __launch_bounds__(JOIN_T) void k_join(JoinArgs g) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    // x keys in range, of those in y, results, their sum, counts added to dst, failed inserts
    unsigned long long n_x = 0, n_both = 0, n_out = 0, sum_out = 0, added = 0, n_fail = 0;
    for (uint64_t bkt = (uint64_t)blockIdx.x * JOIN_T + threadIdx.x; bkt < g.x.nbuckets;
         bkt += (uint64_t)gridDim.x * JOIN_T) {
        uint64_t bw[BUCKET_WORDS];
        load_bucket(g.x.buckets + bkt * BUCKET_WORDS, bw);
#pragma unroll
        for (int sl = 0; sl < S; sl++) {
            if (bw[sl * W] == EMPTY) continue;
            const uint64_t cw = bw[S * W + sl];
            if (!in_range(tc_of(cw, g.mode_x), g.x_min, g.x_max)) continue;
            uint64_t tk[W];
#pragma unroll
            for (int i = 0; i < W; i++) tk[i] = bw[sl * W + i];
            bool found;
            const uint64_t cwy = table_count_word<W>(g.y, tk, found);
            const bool in_y = found && in_range(tc_of(cwy, g.mode_y), g.y_min, g.y_max);
            n_x++;
            n_both += in_y;
            const uint64_t cx = cw & CNT_MASK, cy = in_y ? cwy & CNT_MASK : 0;
            uint64_t r;
            if (g.second) r = in_y ? 0 : join_apply(g.op, 0, cx);  // (x = b: the keys a lacks)
            else r = join_apply(g.op, cx, cy);
            if (!r) continue;
            n_out++;
            sum_out += r;
            if (g.dst.buckets) {
                if (table_insert<W>(g.dst, tk, r)) added += r;
                else n_fail++;
            }
        }
    }
    // (the second launch: x = b, so the keys y = a lacks are b_only; `both` was counted by the first)
    const unsigned long long v[6] = {g.second ? n_x - n_both : n_x, g.second ? 0 : n_both, n_out, sum_out, added, n_fail};
    // the statistics (a_keys or, for the second launch, b_only; both; out_keys; out_sum) and dst's counters
    unsigned long long* const st = g.stats;
    unsigned long long* const dst[6] = {st ? st + (g.second ? 2 : 0) : nullptr, st ? st + 1 : nullptr,
                                        st ? st + 3 : nullptr, st ? st + 4 : nullptr,
                                        g.ctr ? &g.ctr->inserted : nullptr, g.ctr ? &g.ctr->overflow : nullptr};
    block_sum_add<6>(v, dst);
}

template <int W>
hipError_t JoinOps<W>::join(TableView x, TableView y, TableView dst, int mode_x, int mode_y, uint32_t x_min,
                            uint32_t x_max, uint32_t y_min, uint32_t y_max, int op, int second, DevCounters* ctr,
                            unsigned long long* stats, hipStream_t s) {
    if (!x.nbuckets) return hipSuccess;
    const JoinArgs g{x, y, dst, mode_x, mode_y, x_min, x_max, y_min, y_max, op, second, ctr, stats};
    const uint64_t need = (x.nbuckets + JOIN_T - 1) / JOIN_T;
    const unsigned grid = (unsigned)(need < JOIN_BLOCKS ? need : JOIN_BLOCKS);
    hipLaunchKernelGGL(k_join<W>, dim3(grid), dim3(JOIN_T), 0, s, g);
    return hipGetLastError();
}

}  // namespace kc
