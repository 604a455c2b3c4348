// kc_correct_impl.h -- read correction from the counted table (kc_correct*), the kernel for one key
// width W (instantiated by kc_correct_w.hip): k_correct_try, which tries the three other bases at
// every candidate position.  The width-independent kernels (mark, apply) are in kc_correct.hip; the
// rule is the one of include/kc_api.h.  The reference has no counterpart.
//
// A wave owns 64 consecutive positions of the pass.  Two stages:
//  1. every candidate lane on its own: ONE covering window, extracted once (extract_window: no
//     rolling, no key in HBM), its candidate symbol XOR-patched to each of the three other bases,
//     made canonical and looked up with lookup_thread -- three lookups.  An alternative that is weak
//     in this window does not work, and that is almost every alternative of almost every
//     candidate: in a read with one error all the positions the weak windows cover alone are
//     candidates and only one of them is the error.
//  2. the wave together on each candidate that still has an alternative, one after the other: the
//     candidate's covering windows [lo, hi] (at most k, clamped to its sequence) go over the lanes,
//     64 per round, and one ballot per round ends an alternative at its first round with a weak
//     window; the right one takes ceil(|C(p)| / 64) rounds.
// No lane runs a serial loop of dependent lookups longer than 3 + 3 * ceil(k / 64).
// -DKC_CORRECT_NO_PREFILTER builds the kernel without stage 1 (every candidate, all three
// alternatives, goes to stage 2): the form measured against in DESIGN.md 3a.
//
// Like the lookups the kernel only reads the table (kc_table_read.h): plain loads, the READY flag
// masked.
#pragma once
#include "kc_correct_seq.h"
#include "kc_query_impl.h"

namespace kc {

// T of the window fwd (starting at w) with the symbol of position pc >= w XOR-ed with d
template <int W>
DEV uint32_t correct_patched_count(const TableView& tv, const uint64_t (&fwd)[W], const RollConst& rk, uint64_t w,
                                   uint64_t pc, int d, int count_mode) {
    const int bit = 2 * (rk.k - 1 - (int)(pc - w));  // the symbol's place in the 2k-bit integer
    const int wi = W - 1 - (bit >> 6);
    uint64_t f[W], rc[W], key[W], t[W];
#pragma unroll
    for (int j = 0; j < W; j++) f[j] = j == wi ? fwd[j] ^ ((uint64_t)d << (bit & 63)) : fwd[j];
    revcomp<W>(f, rk, rc);
    canonical<W>(f, rc, key);
    to_tkey<W>(key, t);
    return lookup_thread<W>(tv, t, count_mode);
}

// verdict[p] of the pass's n_pos positions: CV_CAND positions (k_correct_mark) become CV_CAND alone
// (no alternative works), CV_CAND | CV_AMBIG (two or three work) or CV_CAND | CV_ACC | y (exactly
// one: the base code y).  sv, cnt: the pass's packed stream and per-position counts; off: the
// sequences' offsets (text bytes; the pass starts at byte `base` and holds sequences i0 .. i1 - 1).
template <int W>
__global__ __launch_bounds__(256) void k_correct_try(TableView tv, PackedView sv, const uint32_t* __restrict__ cnt,
                                                     uint64_t n_pos, uint64_t base, const uint64_t* __restrict__ off,
                                                     uint64_t i0, uint64_t i1, int k, int count_mode, uint32_t smin,
                                                     uint8_t* __restrict__ verdict) {
    const int lane = threadIdx.x & 63;
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t p0 = p - lane;
    if (p0 >= n_pos) return;  // the whole wave is past the end (wave-uniform)
    const uint8_t mine = p < n_pos ? verdict[p] : 0;
    if (!__ballot(mine & CV_CAND)) return;
    const RollConst rk = make_roll<W>(k, 0, 0);
    uint32_t alive = (mine & CV_CAND) ? 0xEu : 0u;  // bit d: the alternative code(text[p]) ^ d may work
#ifndef KC_CORRECT_NO_PREFILTER
    if (alive) {  // stage 1: the first window of C(p)
        const uint64_t i = correct_seq_of(off, i0, i1, base + p);
        uint64_t lo = 0, hi = 0, fwd[W];
        correct_cover(off[i] - base, off[i + 1] - base, p, k, lo, hi);  // (a candidate has covering windows)
        while (lo < hi && cnt[lo] == KC_NO_KMER) lo++;
        alive = 0;
        if (extract_window<W>(sv, lo + (uint64_t)k - 1, rk, fwd)) {
#pragma unroll 1
            for (int d = 1; d <= 3; d++)
                if (correct_patched_count<W>(tv, fwd, rk, lo, p, d, count_mode) >= smin) alive |= 1u << d;
        }
    }
#endif
    uint64_t todo = __ballot(alive != 0);
    uint8_t res = mine;
    while (todo) {  // stage 2 (wave-uniform: every lane works on candidate pc)
        const int src = __ffsll((unsigned long long)todo) - 1;
        todo &= todo - 1;
        const uint32_t al = __shfl(alive, src, 64);
        const uint64_t pc = p0 + src;
        const uint64_t i = correct_seq_of(off, i0, i1, base + pc);
        uint64_t lo = 0, hi = 0;
        correct_cover(off[i] - base, off[i + 1] - base, pc, k, lo, hi);
        int works = 0, which = 0;
#pragma unroll 1
        for (int d = 1; d <= 3; d++) {
            if (!((al >> d) & 1)) continue;
            bool fail = false;
            for (uint64_t w0 = lo; w0 <= hi && !fail; w0 += 64) {
                const uint64_t w = w0 + lane;
                bool weak = false;
                uint64_t fwd[W];
                if (w <= hi && cnt[w] != KC_NO_KMER && extract_window<W>(sv, w + (uint64_t)k - 1, rk, fwd))  // a window of C(pc)
                    weak = correct_patched_count<W>(tv, fwd, rk, w, pc, d, count_mode) < smin;
                fail = __ballot(weak) != 0;
            }
            if (!fail) {
                works++;
                which = d;
            }
        }
        if (lane == src) {
            if (works == 1)
                res = (uint8_t)(CV_CAND | CV_ACC | (sym_at(sv, pc) ^ (uint32_t)which));
            else if (works > 1)
                res = CV_CAND | CV_AMBIG;
        }
    }
    if (res != mine) verdict[p] = res;
}

template <int W>
hipError_t CorrectOps<W>::attempt(TableView t, PackedView sv, const uint32_t* counts, uint64_t n_pos, uint64_t base,
                                  const uint64_t* off, uint64_t i0, uint64_t i1, int k, int count_mode, uint32_t smin,
                                  uint8_t* verdict, hipStream_t s) {
    if (!n_pos) return hipSuccess;
    hipLaunchKernelGGL(k_correct_try<W>, dim3((unsigned)((n_pos + 255) / 256)), dim3(256), 0, s, t, sv, counts, n_pos,
                       base, off, i0, i1, k, count_mode, smin, verdict);
    return hipGetLastError();
}

}  // namespace kc
