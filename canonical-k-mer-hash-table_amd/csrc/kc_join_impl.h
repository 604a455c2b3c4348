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
// X and Y are only read and are ordered after their counting passes, so every stored key is
// published: plain loads, no atomics, no READY spinning (the flag is masked off the count word),
// as kc_query_impl.h argues.  A probe ends at the first bucket with a free slot.  dst is written
// by table_insert's CAS / atomic adds alone, so inserts of several launches and of other writers
// of dst on the same stream order add up.
//
// Statistics and dst's counters are reduced per workgroup: one atomic per non-zero field per
// workgroup; the grid is capped and strides over the buckets, so a C2-sized table (31 M buckets)
// issues a few thousand atomics per field, not 10^5.
#pragma once
#include "kc_common.h"
#include "kc_query_impl.h"
#include "kc_table_insert.h"

namespace kc {

constexpr int JOIN_T = 256;
constexpr uint64_t JOIN_BLOCKS = 4096;  // grid-stride: 16 workgroups per CU

// the count word of table key t in tv (found = false: the table does not hold it)
template <int W>
DEV uint64_t join_probe(const TableView& tv, const uint64_t (&t)[W], bool& found) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    const uint64_t region = region_of(t[0], tv.R);
    uint32_t b = bucket_in_region(t[0], tv.R);
    found = false;
    for (int probe = 0; probe < BPR; probe++) {
        const uint64_t* bk = tv.buckets + (region * BPR + b) * BUCKET_WORDS;
        bool free = false;
        if constexpr (W == 1) {  // the whole bucket: the count word arrives with the keys
            uint64_t bw[BUCKET_WORDS];
            query_load_bucket(bk, bw);
            uint64_t cw = 0;
#pragma unroll
            for (int sl = 0; sl < S; sl++) {
                free |= bw[sl] == EMPTY;
                if (bw[sl] == t[0]) {
                    found = true;
                    cw = bw[S + sl];
                }
            }
            if (found) return cw;
        } else {
#pragma unroll
            for (int sl = 0; sl < S; sl++) {
                const uint64_t w0 = bk[sl * W];
                free |= w0 == EMPTY;
                if (w0 != t[0]) continue;
                bool eq = true;
#pragma unroll
                for (int i = 1; i < W; i++) eq &= bk[sl * W + i] == t[i];
                if (eq) {
                    found = true;
                    return bk[S * W + sl];
                }
            }
        }
        if (free) return 0;
        b = (b + 1) & (BPR - 1);
    }
    return 0;
}

DEV bool join_in_range(uint32_t tc, uint32_t lo, uint32_t hi) { return tc >= lo && (hi == 0 || tc <= hi); }

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

// the workgroup's sums of six per-thread values, one atomic per non-zero sum: into the statistics
// (st, may be null: a_keys or, for the second launch, b_only; both; out_keys; out_sum) and into
// dst's counters (ctr, may be null: inserted, overflow)
DEV void join_block_add(const unsigned long long (&v)[6], unsigned long long* st, int second, DevCounters* ctr) {
    __shared__ unsigned long long s_red[6][JOIN_T / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < 6; q++) {
        unsigned long long x = v[q];
        for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
        if (lane == 0) s_red[q][wid] = x;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 6) {
        unsigned long long x = 0;
#pragma unroll
        for (int w = 0; w < JOIN_T / 64; w++) x += s_red[t][w];
        unsigned long long* dst;
        if (t < 4) dst = st ? st + (t == 0 ? (second ? 2 : 0) : t == 1 ? 1 : t + 1) : nullptr;
        else dst = ctr ? (t == 4 ? &ctr->inserted : &ctr->overflow) : nullptr;
        if (x && dst) atomicAdd(dst, x);
    }
}

template <int W>
__global__ __launch_bounds__(JOIN_T) void k_join(JoinArgs g) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    // x keys in range, of those in y, results, their sum, counts added to dst, failed inserts
    unsigned long long n_x = 0, n_both = 0, n_out = 0, sum_out = 0, added = 0, n_fail = 0;
    for (uint64_t bkt = (uint64_t)blockIdx.x * JOIN_T + threadIdx.x; bkt < g.x.nbuckets;
         bkt += (uint64_t)gridDim.x * JOIN_T) {
        uint64_t bw[BUCKET_WORDS];
        query_load_bucket(g.x.buckets + bkt * BUCKET_WORDS, bw);
#pragma unroll
        for (int sl = 0; sl < S; sl++) {
            if (bw[sl * W] == EMPTY) continue;
            const uint64_t cw = bw[S * W + sl];
            if (!join_in_range(tc_of(cw, g.mode_x), g.x_min, g.x_max)) continue;
            uint64_t tk[W];
#pragma unroll
            for (int i = 0; i < W; i++) tk[i] = bw[sl * W + i];
            bool found;
            const uint64_t cwy = join_probe<W>(g.y, tk, found);
            const bool in_y = found && join_in_range(tc_of(cwy, g.mode_y), g.y_min, g.y_max);
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
    join_block_add(v, g.stats, g.second, g.ctr);
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
