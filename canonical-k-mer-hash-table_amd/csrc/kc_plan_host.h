// kc_plan_host.h -- the host arithmetic of the partition buffers (kc_api.cpp part_plan) and of the
// packed-stream pass (kc_api_pass.cpp packed_pass): the sizes of a partitioned batch, the window
// bound they are sized for, the cut length of a packed pass and the window count of a break-word
// range.  Plain C++ without a device call or an environment read, so a stand-alone program checks
// it under the sanitizers (tools/plan_host_check.cpp).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>

namespace kc {

constexpr int COUNT_THREADS = 256;
// Windows rolled per thread in the partitioned kernels, and the workgroup size of the
// segmented level 1 (tile = threads x windows), by key width: wide keys take fewer
// windows per thread and smaller groups so that the registers and the LDS tile fit.
constexpr int run_width(int W) { return W == 1 ? 16 : W == 2 ? 8 : W <= 4 ? 8 : 4; }
// The segmented level 1 (k_p1) of one- to four-word keys: 512-thread workgroups, two per CU.
// (1024 threads with half the windows per thread -- 8 waves per SIMD within 64 VGPRs -- spill
// and ran 30 % slower: profiles/r03_ab_p1_nt.txt)
constexpr int scatter_threads_w(int W) { return W <= 4 ? 512 : 256; }
constexpr int p1_runw(int W) { return run_width(W); }
constexpr int p1_tile(int W) { return scatter_threads_w(W) * p1_runw(W); }  // windows per segmented level-1 tile
// Two-word keys may take a 1024-thread level 1 (kc_internal.h p1_wide)
constexpr int P1_WIDE_THREADS = 1024;
// the largest level-1 tile a table pass of W-word keys may run (the host's segment sizing rounds
// block ranges to it)
constexpr int p1_tile_max(int W) { return W == 2 ? P1_WIDE_THREADS * p1_runw(W) : p1_tile(W); }

// geometry of a partitioned pass: F1 coarse bins x F2 regions each (R regions), IW
// u64 words per item
struct PartGeo {
    uint32_t F1, F2;
    uint64_t R;
    int IW;
};
// The sizes of a partitioned pass over a batch of up to `syms` symbols (no allocation):
// level-1 workgroups, level-2 segments per bin, the segment capacities, the skew list and the key
// buffers' words.  slots > 1: the level-2 histogram and key buffers hold that many batches'
// segments (a deferred level 3, run_deferred), each record rec2 bytes (level2_record_bytes)
struct PartPlan {
    uint32_t nblk1, B2;
    uint64_t n1, n2, nbs;     // histogram entries: level 1, level 2, block sums
    uint64_t cap1, cap2;      // segment capacities (0: the exact layout)
    uint64_t spill_cap, spill_words, need1, need2;
};
// the capacities a test forces (KC_SEG_CAP, KC_SPILL_CAP: read by the caller)
struct PlanKnobs {
    bool has_seg_cap = false, has_spill_cap = false;
    uint64_t seg_cap = 0, spill_cap = 0;
};

// The windows a batch of `syms` symbols is planned for at `density` windows per symbol (1: tokenized
// input, where every symbol can end a window).  The exact pipeline writes every valid window of
// the batch into both key buffers without a capacity check, so the density must not be below the
// batch's true one (device_pass: the estimate pass's; packed_pass: packed_batch_density).
inline uint64_t plan_window_bound(uint64_t syms, double density) {
    return density < 1.0 ? (uint64_t)((double)syms * density) + 1024 : syms;
}

// part_plan's arithmetic (kc_api.cpp): W key words, items of g.IW words
inline PartPlan plan_partition(int W, uint64_t syms, double density, bool seg, const PartGeo& g, uint32_t bins1,
                               uint32_t slots, uint64_t rec2, bool tight, const PlanKnobs& kn) {
    PartPlan p{};
    const uint64_t tile = (uint64_t)COUNT_THREADS * run_width(W);
    p.nblk1 = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(2048, (syms + tile - 1) / tile));
    p.B2 = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(64, 2048 / g.F1));
    // every array is sized for the geometry of THIS call (a Bloom job re-sizes the table
    // after each Bloom pass, so F1 and R may grow between calls on one context)
    p.n1 = (uint64_t)std::max<uint32_t>(g.F1, bins1) * 2048;  // level-1 bins x max workgroups
    p.n2 = g.R * p.B2 * slots;
    p.nbs = (std::max(p.n1, p.n2) + 4095) / 4096 + 2;
    if (seg) {
        // tight (a deferred pass): e + 3.5 sigma + 8.  Its keys past a segment's end (a few segments
        // in 10^4 overflow, by a few keys) join the group's skew list, which is inserted once after
        // the group's level 3 (run_deferred), so the slots of more batches fit beside the table (C5
        // on one GPU: 54.2 -> 43.4 GB per batch, groups of 2 -> 3).  (At 3 sigma, C5's ~54 K spilled
        // keys per batch touched ~100 K regions per group in the list's level 3: 12 ms per job.)
        const double sd = tight ? 3.5 : 8.0, add = tight ? 8.0 : 32.0;
        auto capacity = [&](double e) { return ((uint64_t)std::ceil(e + sd * std::sqrt(e) + add) + 7) / 8 * 8; };
        const uint64_t t1 = (uint64_t)p1_tile_max(W);  // k_p1<..., OutSeg> rounds block ranges to its tile
        const uint64_t per1 = ((syms + p.nblk1 - 1) / p.nblk1 + t1 - 1) / t1 * t1;  // symbols per level-1 block
        const uint64_t nseg = (p.nblk1 + p.B2 - 1) / p.B2;                           // level-1 segments per p2 block
        const double d = density;  // windows per symbol
        p.cap1 = capacity((double)per1 * d / g.F1);
        p.cap2 = capacity((double)nseg * per1 * d / g.F1 / g.F2);
        if (kn.has_seg_cap) p.cap1 = p.cap2 = std::max<uint64_t>(1, kn.seg_cap);
        // the segment walks index a virtual run with 32-bit offsets
        if (nseg * p.cap1 >= (1ULL << 31) || (uint64_t)p.B2 * p.cap2 * slots >= (1ULL << 31)) p.cap1 = p.cap2 = 0;
    }
    // the skew list of a segmented batch: {key words, count} records of keys past a segment's
    // end and of repeated windows (Bloom pass: plain keys), an eighth of the windows before the
    // batch falls back to the exact layout; its exact pipeline runs through the key buffers
    const uint64_t wins = plan_window_bound(syms, density);
    if (p.cap1) {
        // (a deferred pass's list takes its group's few spilled keys: a sixteenth)
        p.spill_cap = std::max<uint64_t>(1 << 16, wins / (tight ? 16 : 8));
        if (kn.has_spill_cap) p.spill_cap = kn.spill_cap;  // tests
    }
    p.spill_words = p.spill_cap * (g.IW + 1);
    p.need1 = std::max(std::max<uint64_t>(wins, (uint64_t)g.F1 * p.nblk1 * p.cap1) * g.IW, p.spill_words);
    // one batch's level 2 in W-word items; a deferred group's slots in level-2 records (the exact
    // pipeline of a batch's tail, which writes W-word items, runs after its group's level 3)
    const uint64_t l2 = slots > 1 && rec2 ? (g.R * p.B2 * p.cap2 * slots * rec2 + 7) / 8 : g.R * p.B2 * p.cap2 * g.IW;
    p.need2 = std::max(std::max<uint64_t>(wins * g.IW, l2), p.spill_words);
    // (the levels' record loads are 12 or 16 bytes wide whatever the record: a last 8- or
    // 12-byte record's load reads past it)
    p.need1 += 2;
    p.need2 += 2;
    return p;
}

// ---- the packed-stream pass (kc_count_packed_device / kc_bloom_packed_device) ----------------------
// The caller's `windows` argument is a hint and only chooses the cut length: batches of about a
// staging batch's windows if the stream were uniform, i.e. batch_bytes / (1.15 x windows per
// symbol) symbols, at least 1024 words; 0 = unknown (one window per symbol).
inline double packed_hint_density(uint64_t n_words, uint64_t windows) {
    const double nsym = (double)n_words * 32.0;
    return windows && n_words ? std::min(1.0, 1.15 * (double)windows / nsym + 1e-3) : 1.0;
}
inline uint64_t packed_cut_words(uint64_t batch_bytes, uint64_t n_words, uint64_t windows) {
    return std::max<uint64_t>(1024, (uint64_t)((double)batch_bytes / packed_hint_density(n_words, windows)) / 32);
}

// What sizes the buffers is each batch's counted windows (k_packed_windows over its break words):
// windows per symbol of one batch with a margin for the rounding (as the estimate pass's kept
// batches, kc_estimate_distinct_device), so that plan_window_bound(syms, d) >= windows.  The pass
// plans every batch at the largest of its batches' densities (a deferred group's slots share one
// geometry).  The trivial alternative, sizing the exact buffers for one window per symbol, is not
// acceptable: a C4 owner share at 8 ranks holds ~3.4 symbols per window, and its two key buffers
// would grow from ~24 GB to ~68 GB each.
inline double packed_batch_density(uint64_t windows, uint64_t syms) {
    return std::min(1.0, (double)windows / (double)std::max<uint64_t>(1, syms) * 1.02 + 0.005);
}
// the density a packed pass plans with: measured, never the hint's
inline double packed_plan_density(double hint_density, double measured_density) {
#ifdef KC_PLAN_MUTANT_HINT_DENSITY  // (tools/plan_host_check.cpp's mutation check: the rule before the counter)
    (void)measured_density;
    return hint_density;
#else
    (void)hint_density;
    return measured_density;
#endif
}

// Windows of the break words bk[0 .. n_words): symbols that are no break and have at least k - 1
// break-free predecessors inside the range, i.e. the sum of max(0, L - k + 1) over the maximal
// break-free runs of length L (the symbol before the range counts as a break, as the levels start
// a stream; the range ends at its last word).  The host form of k_packed_windows (kc_util.hip).
inline uint64_t packed_windows_host(const uint32_t* bk, uint64_t n_words, int k) {
    uint64_t n = 0, run = 0;
    for (uint64_t w = 0; w < n_words; w++)
        for (int j = 0; j < 32; j++) {
            run = (bk[w] >> (31 - j)) & 1 ? 0 : run + 1;
            n += run >= (uint64_t)k;
        }
    return n;
}

}  // namespace kc
