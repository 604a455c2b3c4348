// kc_query_impl.h -- queries of the counted full-key table, kernels for one key width W
// (instantiated by kc_query_w.hip): k_lookup, the count T(c) of given k-mers, and k_histo, the
// count-of-counts (abundance spectrum) of the whole table.  The reference has no counterpart:
// its table is only ever walked by the writers (kmer_hash_table.cpp:4318-4524).
//
// Both kernels only read the table, by the rules of kc_table_read.h: plain loads, and a probe that
// ends at the first bucket with a free slot, so a lookup is normally one 128-byte bucket read,
// present or absent.
//
// k_lookup has two forms:
//  * cooperative (W <= 2, the default): a group of 16 lanes reads a bucket as one coalesced
//    128-byte request, one u64 each, and finds the slot with a wave ballot; the count word is
//    a lane shuffle away (the group holds the whole bucket).  Every lane first canonicalises
//    and mixes its own key; the wave then takes 16 steps of four keys (one per group).
//  * one thread per key (W >= 3, and W <= 2 with -DKC_QUERY_TPK): lookup_thread, S <= 4 strided
//    key loads per bucket, the count word only on a hit.
#pragma once
#include "kc_table_read.h"

namespace kc {

// the table key of query i; false: not a k-mer / not a table key (the answer is 0)
template <int W>
DEV bool query_tkey(const uint64_t* __restrict__ keys, uint64_t i, int k, int layout, uint64_t (&t)[W]) {
    uint64_t q[W];
#pragma unroll
    for (int j = 0; j < W; j++) q[j] = keys[i * W + j];
    if (layout == KC_KEYS_TABLE) {
#pragma unroll
        for (int j = 0; j < W; j++) t[j] = q[j];
        return q[0] != EMPTY;
    }
    const RollConst rk = make_roll<W>(k, 0, 0);
    if (q[0] & ~rk.topmask) return false;  // a bit above 2k - 1
    uint64_t rc[W], key[W];
    revcomp<W>(q, rk, rc);
    canonical<W>(q, rc, key);
    to_tkey<W>(key, t);
    return true;
}

// T(c) of table key t, 0 when the table does not hold it.  table_probe's loop (kc_table_read.h),
// kept here as a loop of its own: through table_probe the address arithmetic of k_seq_counts and
// k_correct_try comes out differently (no other register count, but correct_time.py's figures
// 0.5 - 1.6 % up, outside the parent's own spread); with this loop the query, sequence and
// correction units compile to the code they had.
template <int W>
DEV uint32_t lookup_thread(const TableView& tv, const uint64_t (&t)[W], int count_mode) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    const uint64_t region = region_of(t[0], tv.R);
    uint32_t b = bucket_in_region(t[0], tv.R);
    for (int probe = 0; probe < BPR; probe++) {
        const uint64_t* bk = tv.buckets + (region * BPR + b) * BUCKET_WORDS;
        bool free = false;
#pragma unroll
        for (int sl = 0; sl < S; sl++) {
            const uint64_t w0 = bk[sl * W];
            free |= w0 == EMPTY;
            if (w0 != t[0]) continue;
            bool eq = true;
#pragma unroll
            for (int i = 1; i < W; i++) eq &= bk[sl * W + i] == t[i];
            if (eq) return tc_of(bk[S * W + sl], count_mode);
        }
        if (free) return 0;
        b = (b + 1) & (BPR - 1);
    }
    return 0;
}

template <int W>
__global__ __launch_bounds__(256) void k_lookup_tpk(TableView tv, int k, int count_mode, int layout,
                                                    const uint64_t* __restrict__ keys, uint64_t n,
                                                    uint32_t* __restrict__ counts) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    uint64_t t[W];
    const bool ok = query_tkey<W>(keys, i, k, layout, t);
    counts[i] = ok ? lookup_thread<W>(tv, t, count_mode) : 0;
}

// cooperative form: 16 lanes per bucket, four keys per wave per step (W <= 2); the probe is
// table_probe's (kc_table_read.h), a bucket across 16 lanes
template <int W>
__global__ __launch_bounds__(256) void k_lookup_coop(TableView tv, int k, int count_mode, int layout,
                                                     const uint64_t* __restrict__ keys, uint64_t n,
                                                     uint32_t* __restrict__ counts) {
    static_assert(W <= 2, "the group compares at most two words per slot");
    constexpr int S = BUCKET_WORDS / (W + 1);
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (i - lane >= n) return;  // the whole wave is past the end (wave-uniform)
    uint64_t t[W];
#pragma unroll
    for (int j = 0; j < W; j++) t[j] = 0;
    const bool mine = i < n && query_tkey<W>(keys, i, k, layout, t);
    const int g0 = lane & 48, sub = lane & 15;
    // the words of a bucket that hold word 0 / word 1 of a slot's key
    const bool is_k0 = sub < S * W && (W == 1 || !(sub & 1));
    const bool is_k1 = W == 2 && sub < S * W && (sub & 1);
    uint32_t res = 0;
    for (int r = 0; r < 16; r++) {
        const int src = g0 | r;  // this step's key of the group
        const uint64_t t0 = __shfl(t[0], src, 64);
        const uint64_t t1 = W == 2 ? __shfl(t[W - 1], src, 64) : 0;
        bool act = __shfl((int)mine, src, 64) != 0;
        const uint64_t region = region_of(t0, tv.R);
        uint32_t b = bucket_in_region(t0, tv.R);
        uint32_t found = 0;
        for (int probe = 0; probe < BPR && __ballot(act); probe++) {
            uint64_t w = 0;
            if (act) w = tv.buckets[(region * BPR + b) * BUCKET_WORDS + sub];
            uint64_t bm = __ballot(act && is_k0 && w == t0);
            if constexpr (W == 2) bm &= __ballot(act && is_k1 && w == t1) >> 1;
            const uint64_t bf = __ballot(act && is_k0 && w == EMPTY);
            const uint32_t gm = (uint32_t)(bm >> g0) & 0xFFFF, gf = (uint32_t)(bf >> g0) & 0xFFFF;
            // the count word of the matching slot: every lane takes part in the shuffle
            const int slot = gm ? (__ffs((int)gm) - 1) / W : 0;
            const uint64_t cw = __shfl(w, g0 | (S * W + slot), 64);
            if (act && gm) found = tc_of(cw, count_mode);
            if (gm || gf) act = false;
            b = (b + 1) & (BPR - 1);
        }
        if (sub == r) res = found;
    }
    if (i < n) counts[i] = res;
}

// k_histo: hist[min(T(c), n_bins - 1)] += 1 for every occupied slot.  One sweep of the table, a
// bucket per thread (as k_dump); the bins below HISTO_LDS_BINS are counted per workgroup in LDS
// and flushed with one global atomic per non-zero bin, the rare larger values go straight to
// global atomics.
constexpr uint32_t HISTO_LDS_BINS = 8192;  // 32 KiB of u32 bins
constexpr int HISTO_T = 256;
constexpr uint64_t HISTO_BLOCKS = 1024;    // grid-stride: four workgroups per CU, one flush each
template <int W>
__global__ __launch_bounds__(HISTO_T) void k_histo(TableView tv, int count_mode, uint32_t n_bins,
                                                   unsigned long long* __restrict__ hist) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    __shared__ uint32_t s_bins[HISTO_LDS_BINS];
    const uint32_t nl = n_bins < HISTO_LDS_BINS ? n_bins : HISTO_LDS_BINS;
    for (uint32_t j = threadIdx.x; j < nl; j += HISTO_T) s_bins[j] = 0;
    __syncthreads();
    for (uint64_t bkt = (uint64_t)blockIdx.x * HISTO_T + threadIdx.x; bkt < tv.nbuckets;
         bkt += (uint64_t)gridDim.x * HISTO_T) {
        uint64_t bw[BUCKET_WORDS];
        load_bucket(tv.buckets + bkt * BUCKET_WORDS, bw);
#pragma unroll
        for (int s = 0; s < S; s++) {
            if (bw[s * W] == EMPTY) continue;
            uint32_t v = tc_of(bw[S * W + s], count_mode);
            if (v > n_bins - 1) v = n_bins - 1;
            if (v < HISTO_LDS_BINS)
                atomicAdd(&s_bins[v], 1u);
            else
                atomicAdd(&hist[v], 1ULL);
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < nl; j += HISTO_T) {
        const uint32_t c = s_bins[j];
        if (c) atomicAdd(&hist[j], (unsigned long long)c);
    }
}

template <int W>
hipError_t QueryOps<W>::lookup(TableView t, int k, int count_mode, int layout, const uint64_t* keys, uint64_t n,
                               uint32_t* counts, hipStream_t s) {
    if (!n) return hipSuccess;
    const dim3 grid((unsigned)((n + 255) / 256));
#ifndef KC_QUERY_TPK
    if constexpr (W <= 2) {
        hipLaunchKernelGGL(k_lookup_coop<W>, grid, dim3(256), 0, s, t, k, count_mode, layout, keys, n, counts);
        return hipGetLastError();
    }
#endif
    hipLaunchKernelGGL(k_lookup_tpk<W>, grid, dim3(256), 0, s, t, k, count_mode, layout, keys, n, counts);
    return hipGetLastError();
}

template <int W>
hipError_t QueryOps<W>::histo(TableView t, int count_mode, uint32_t n_bins, unsigned long long* hist,
                              hipStream_t s) {
    if (!t.nbuckets) return hipSuccess;
    const uint64_t need = (t.nbuckets + HISTO_T - 1) / HISTO_T;
    const unsigned grid = (unsigned)(need < HISTO_BLOCKS ? need : HISTO_BLOCKS);
    hipLaunchKernelGGL(k_histo<W>, dim3(grid), dim3(HISTO_T), 0, s, t, count_mode, n_bins, hist);
    return hipGetLastError();
}

}  // namespace kc
