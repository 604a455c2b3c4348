// kc_seq_impl.h -- sequence queries of the counted full-key table, the kernel for one key width W
// (instantiated by kc_seq_w.hip): k_seq_counts, T(c) of the canonical k-mer that starts at every
// position of a text.  The reference has no counterpart (its table is only walked by the writers).
//
// The text arrives as a position-preserving packed stream (kc_seq.hip k_seq_pack: symbol p = byte
// p, every non-ACGT byte a break).  A thread takes the run_width(W) consecutive window starts
// s0 .. s0 + RUNW - 1, i.e. the windows ending at s0 + k - 1 ..: run_windows extracts the first
// in O(1) and rolls the rest, each is made canonical, mixed into its table key and looked up with
// lookup_thread (kc_query_impl.h; the probe's rules: kc_table_read.h).  No key goes through HBM.  The answers are written at the
// windows' start positions, RUNW consecutive uint32 per thread, so a wave's stores cover one
// contiguous range.
//
// Two forms of the lookup inside the kernel were built and measured (tools/seq_probe.py):
// one thread per key (lookup_thread) for every width is the default (suspected reason: a thread's
// RUNW lookups are independent, so several bucket reads per lane are in flight); the cooperative form (16 lanes per
// bucket, every lane of the wave stepping through the run in lockstep: 16 x RUNW serial steps per
// wave) is 19-23 % slower here for one- and two-word keys, although it is the faster one in
// k_lookup_coop, where a lane has one key.  -DKC_SEQ_COOP_MAX_W=2 builds it.
//
// Like the lookups the kernel only reads the table: plain loads, the READY flag masked.
#pragma once
#include "kc_query_impl.h"

namespace kc {

// The probe loop of k_lookup_coop (kc_query_impl.h) as a device function (the variant build): every lane of the wave
// calls it with its own table key (mine: it has one) and gets that key's T(c) back.  16 lanes read
// a bucket as one 128-byte request; the wave takes 16 steps of four keys.  (k_lookup_coop keeps
// its own copy of the loop: calling this function from it changes the register allocation of a
// kernel whose code and measurements stay as they are.  Both walk the probe sequence of
// kc_table_read.h and end by its invariant; table_probe there is the form of one thread per key.)
template <int W>
DEV uint32_t lookup_coop(const TableView& tv, const uint64_t (&t)[W], bool mine, int count_mode, int lane) {
    static_assert(W <= 2, "the group compares at most two words per slot");
    constexpr int S = BUCKET_WORDS / (W + 1);
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
    return res;
}

// the widest key looked up cooperatively (0: none, the default; -DKC_SEQ_COOP_MAX_W=1 / 2: the A/B of
// tools/seq_probe.py)
#ifndef KC_SEQ_COOP_MAX_W
#define KC_SEQ_COOP_MAX_W 0
#endif
constexpr int SEQ_COOP_MAX_W = KC_SEQ_COOP_MAX_W;

// counts[p], p < n_pos: T(c) of the window sv[p, p + k) if it holds no break and p + k <= n_sym,
// else KC_NO_KMER.  sv holds seq_pack_words(n_sym) words; n_sym >= k (the launcher answers a
// shorter stream itself).
template <int W>
__global__ __launch_bounds__(256) void k_seq_counts(TableView tv, PackedView sv, int k, int count_mode, uint64_t n_pos,
                                                    uint64_t n_sym, uint32_t* __restrict__ counts) {
    constexpr int RW = run_width(W);
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if ((g - lane) * RW >= n_pos) return;  // the whole wave is past the end (wave-uniform)
    const uint64_t s0 = g * RW;
    const RollConst rk = make_roll<W>(k, 0, 0);
    // a thread whose first window already ends past the stream rolls the stream's first run with
    // every window refused (the words it reads exist: n_sym >= k), so that the wave stays whole
    // (the cooperative lookup needs every lane)
    const bool live = s0 < n_pos && s0 + (uint64_t)k - 1 < n_sym;
    const uint64_t r0 = (live ? s0 : 0) + (uint64_t)k - 1;
    const uint64_t t1 = live ? n_sym : 0;
    uint32_t res[RW];
    run_windows<W, RW>(sv, r0, t1, rk, [&](int j, bool ok, const uint64_t (&fwd)[W], const uint64_t (&rc)[W]) {
        uint64_t key[W], t[W];
        canonical<W>(fwd, rc, key);
        to_tkey<W>(key, t);
        uint32_t v;
        if constexpr (W <= SEQ_COOP_MAX_W)
            v = lookup_coop<W>(tv, t, ok, count_mode, lane);
        else
            v = ok ? lookup_thread<W>(tv, t, count_mode) : 0;
        res[j] = ok ? v : KC_NO_KMER;
    });
    if (s0 >= n_pos) return;
    if (s0 + RW <= n_pos && !(reinterpret_cast<uintptr_t>(counts) & 15)) {
        uint4* o = reinterpret_cast<uint4*>(counts + s0);
#pragma unroll
        for (int q = 0; q < RW / 4; q++) o[q] = make_uint4(res[4 * q], res[4 * q + 1], res[4 * q + 2], res[4 * q + 3]);
    } else {
#pragma unroll
        for (int j = 0; j < RW; j++)
            if (s0 + j < n_pos) counts[s0 + j] = res[j];
    }
}

template <int W>
hipError_t SeqOps<W>::counts(TableView t, PackedView sv, int k, int count_mode, uint64_t n_pos, uint64_t n_sym,
                             uint32_t* counts, hipStream_t s) {
    if (!n_pos) return hipSuccess;
    if (n_sym < (uint64_t)k) return hipMemsetAsync(counts, 0xFF, n_pos * sizeof(uint32_t), s);  // KC_NO_KMER everywhere
    const uint64_t threads = (n_pos + run_width(W) - 1) / run_width(W);
    hipLaunchKernelGGL(k_seq_counts<W>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, t, sv, k, count_mode,
                       n_pos, n_sym, counts);
    return hipGetLastError();
}

}  // namespace kc
