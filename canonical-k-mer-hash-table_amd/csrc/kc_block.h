// kc_block.h -- what a workgroup of BLOCK_T = 256 threads (four waves) does together on the read
// side: places behind a shared cursor with one atomic per workgroup or wave, and the workgroup's
// sums of per-thread statistics with one atomic per non-zero sum.  (One cursor word takes about 90
// atomics per microsecond: one per wave and iteration of k_graph_links' sweep, 4 M on a C2 table,
// took 43 ms.)
#pragma once
#include "kc_common.h"

namespace kc {

constexpr int BLOCK_T = 256;

// This thread's first index behind *cursor for its `mine` items, the workgroup's items in thread
// order: one atomic per workgroup, none when the workgroup has no item.  Every thread of the
// workgroup must call it together (two barriers inside).  Its shared words belong to the call
// until every thread has its index: a kernel that calls it again -- the next tile of a sweep --
// puts a barrier of its own between the calls.
DEV uint64_t block_reserve(uint32_t mine, unsigned long long* cursor) {
    __shared__ unsigned long long s_wt[BLOCK_T / 64], s_base;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_sum(mine);
    if (lane == 63) s_wt[wid] = incl;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long tot = s_wt[0] + s_wt[1] + s_wt[2] + s_wt[3];
        s_base = tot ? atomicAdd(cursor, tot) : 0;
    }
    __syncthreads();
    unsigned long long base = s_base;
    for (int w = 0; w < wid; w++) base += s_wt[w];
    return base + incl - mine;
}
static_assert(BLOCK_T / 64 == 4, "block_reserve adds four wave totals");

// The wave's form: this lane's index behind *cursor if flag, the wave's flagged lanes in lane
// order; one atomic per wave, none when no lane is flagged.  The wave's active lanes call it
// together.  (An unflagged lane gets the index of the next flagged one: not a place of its own.)
DEV uint64_t wave_reserve(bool flag, unsigned long long* cursor) {
    const uint64_t ballot = __ballot(flag);
    const int lane = threadIdx.x & 63;
    unsigned long long base = 0;
    if (ballot) {
        const int first = __ffsll((long long)ballot) - 1;
        if (lane == first) base = atomicAdd(cursor, (unsigned long long)__popcll(ballot));
        base = __shfl(base, first, 64);
    }
    return base + __popcll(ballot & ((1ULL << lane) - 1));
}

// *dst[q] += the workgroup's sum of v[q], q < N <= 64: one atomic per non-zero sum with a
// destination (dst[q] null: the sum is dropped).  Every thread of the workgroup calls it together,
// once per kernel (a second call would need a barrier before it).
template <int N>
DEV void block_sum_add(const unsigned long long (&v)[N], unsigned long long* const (&dst)[N]) {
    static_assert(N <= 64, "one thread of the first wave per sum");
    __shared__ unsigned long long s_red[N][BLOCK_T / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < N; q++) {
        unsigned long long x = v[q];
        for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m, 64);
        if (lane == 0) s_red[q][wid] = x;
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < N) {
        unsigned long long x = 0;
#pragma unroll
        for (int w = 0; w < BLOCK_T / 64; w++) x += s_red[t][w];
        unsigned long long* d = nullptr;
#pragma unroll
        for (int q = 0; q < N; q++)
            if (t == q) d = dst[q];
        if (x && d) atomicAdd(d, x);
    }
}

}  // namespace kc
