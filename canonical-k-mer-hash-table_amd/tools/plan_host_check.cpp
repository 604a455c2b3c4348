// plan_host_check -- the host arithmetic of the partition buffers and of the packed-stream pass
// (csrc/kc_plan_host.h) on the CPU, built with -fsanitize=address,undefined (make
// bin/plan_host_check).  Exit status 0 when every check holds.
//
//   1. plan_partition over W = 1..15, batches of one tile to 2^33 symbols, 0.01 to 1 windows per
//      symbol, small and C4-sized geometries, the exact, segmented and tight layouts and forced
//      capacities of 8: both key buffers hold the batch's true windows x item words + the 2-word read
//      slack, need1 covers F1 x nblk1 x cap1 items, need2 the level-2 segments, the skew list fits
//      both, and the capacities are 0 before a 32-bit segment offset can overflow.
//   2. packed_cut_words: at least 1024 words, and monotone in the hint.
//   3. Heterogeneous streams (20 000 sequences of k symbols and 40 of 4991, in both orders, and
//      the dense part in the middle) through packed_pass's cuts with every kind of hint: every
//      batch's buffers hold its windows.  With -DKC_PLAN_MUTANT_HINT_DENSITY (the pass planned at
//      its hint's density, the rule before the windows were counted) these rows must fail.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../csrc/kc_plan_host.h"

using namespace kc;

static long g_checks = 0, g_fails = 0;
#define CHECK(cond, ...)                              \
    do {                                              \
        g_checks++;                                   \
        if (!(cond)) {                                \
            if (g_fails++ < 12) {                     \
                std::printf("FAIL %s: ", #cond);      \
                std::printf(__VA_ARGS__);             \
                std::printf("\n");                    \
            }                                         \
        }                                             \
    } while (0)

struct Layout {
    const char* name;
    bool seg, tight;
    uint32_t slots;
};
static const Layout kLayouts[] = {{"exact", false, false, 1}, {"segmented", true, false, 1}, {"tight", true, true, 3}};

// what every plan must satisfy for a batch of `syms` symbols that holds `wins` windows
static void check_plan(const char* what, int W, const PartGeo& g, uint64_t syms, uint64_t wins, double density,
                       const Layout& l, const PlanKnobs& kn) {
    const uint64_t rec2 = l.slots > 1 ? (W == 1 ? 6 : 8ull * W) : 0;
    const PartPlan p = plan_partition(W, syms, density, l.seg, g, 0, l.slots, rec2, l.tight, kn);
    const uint64_t iw = (uint64_t)g.IW, nseg = (p.nblk1 + p.B2 - 1) / p.B2;
#define ROW "%s W %d IW %d F1 %u F2 %u syms %" PRIu64 " wins %" PRIu64 " d %.4f %s forced %d", what, W, g.IW, g.F1, \
            g.F2, syms, wins, density, l.name, (int)kn.has_seg_cap
    CHECK(plan_window_bound(syms, density) >= wins, ROW);
    CHECK(p.need1 >= wins * iw + 2, ROW);
    CHECK(p.need2 >= wins * iw + 2, ROW);
    CHECK(p.need1 >= (uint64_t)g.F1 * p.nblk1 * p.cap1 * iw + 2, ROW);
    CHECK(p.need2 >= (l.slots > 1 ? (g.R * p.B2 * p.cap2 * l.slots * rec2 + 7) / 8 : g.R * p.B2 * p.cap2 * iw) + 2, ROW);
    CHECK(p.spill_words == p.spill_cap * (iw + 1) && p.spill_words <= p.need1 - 2 && p.spill_words <= p.need2 - 2, ROW);
    CHECK((p.cap1 == 0) == (p.cap2 == 0) && (l.seg || p.cap1 == 0), ROW);
    CHECK(p.cap1 == 0 || (nseg * p.cap1 < (1ULL << 31) && (uint64_t)p.B2 * p.cap2 * l.slots < (1ULL << 31)), ROW);
    CHECK(p.cap1 != 0 || p.spill_cap == 0, ROW);
    CHECK(p.nblk1 >= 1 && p.nblk1 <= 2048 && p.B2 >= 1 && p.n1 >= (uint64_t)g.F1 * p.nblk1 &&
              p.n2 == g.R * p.B2 * l.slots && p.nbs * 4096 >= std::max(p.n1, p.n2),
          ROW);
#undef ROW
}

static void sweep_plans() {
    const uint64_t syms_list[] = {4096, 5000, 1ull << 16, 1000003, 1ull << 24, 1ull << 28, (1ull << 31) + 77, 1ull << 33};
    const double dens_list[] = {0.01, 0.05, 0.30, 0.62, 0.97, 1.0};
    // regions of 64 KiB: a 2 M-slot table, a C4 owner share (271 x 1024), the largest level-1 fan-out
    const PartGeo geos[] = {{1, 1, 1, 0}, {4, 2, 8, 0}, {16, 16, 256, 0}, {271, 1024, 271ull * 1024, 0},
                            {1024, 2048, 1ull << 21, 0}};
    for (int W = 1; W <= 15; W++)
        for (const PartGeo& g0 : geos)
            for (int iw : {1, W, W + 1}) {  // the Bloom pass's hashes, table keys, {key, count} records
                if (iw == 1 && W > 1 && g0.F1 > 16) continue;
                PartGeo g = g0;
                g.IW = iw;
                for (uint64_t syms : syms_list)
                    for (double d : dens_list) {
                        const uint64_t wins = d >= 1.0 ? syms : (uint64_t)((double)syms * d);
                        const double dens = packed_batch_density(wins, syms);
                        for (const Layout& l : kLayouts) {
                            check_plan("sweep", W, g, syms, wins, dens, l, PlanKnobs{});
                            PlanKnobs forced;
                            forced.has_seg_cap = forced.has_spill_cap = true;
                            forced.seg_cap = forced.spill_cap = 8;
                            check_plan("sweep", W, g, syms, wins, dens, l, forced);
                        }
                    }
            }
}

static void sweep_cuts() {
    for (uint64_t bb : {64ull << 10, 64ull << 20, 256ull << 20, 2ull << 30})
        for (uint64_t n_words : {1ull, 1000ull, 31250ull, 1ull << 22, 1ull << 28}) {
            const uint64_t nsym = n_words * 32;
            // hints in growing order; 0 = unknown counts as the largest (one window per symbol)
            const uint64_t hints[] = {1, nsym / 300 + 1, nsym / 30 + 1, nsym / 3 + 1, nsym, 8 * nsym, ~0ull >> 8, 0};
            uint64_t prev = ~0ull;
            for (uint64_t h : hints) {
                const uint64_t lim = packed_cut_words(bb, n_words, h);
                CHECK(lim >= 1024, "cut %" PRIu64 " words: batch %" PRIu64 " n_words %" PRIu64 " hint %" PRIu64, lim, bb,
                      n_words, h);
                CHECK(lim <= prev, "cut not monotone: %" PRIu64 " after %" PRIu64 " (batch %" PRIu64 " n_words %" PRIu64
                      " hint %" PRIu64 ")", lim, prev, bb, n_words, h);
                prev = lim;
            }
            CHECK(packed_cut_words(bb, n_words, 0) == std::max<uint64_t>(1024, bb / 32), "unknown hint: one window per symbol");
        }
}

// the break words of sequences of the given lengths, each preceded by a break symbol, the last
// word padded with breaks (the stream format of kc_route_superkmers_device)
static std::vector<uint32_t> break_words(const std::vector<std::pair<uint64_t, uint64_t>>& seqs, uint64_t* formula,
                                         int k) {
    std::vector<uint32_t> bk;
    uint64_t pos = 0;
    *formula = 0;
    auto put_break = [&]() {
        if (pos / 32 >= bk.size()) bk.push_back(0);
        bk[pos / 32] |= 0x80000000u >> (pos % 32);
        pos++;
    };
    for (auto& s : seqs)
        for (uint64_t i = 0; i < s.second; i++) {
            put_break();
            pos += s.first;
            bk.resize((pos + 31) / 32, 0);
            if (s.first >= (uint64_t)k) *formula += s.first - k + 1;
        }
    while (pos % 32) put_break();
    return bk;
}

static void heterogeneous_rows() {
    const uint64_t batch_bytes = 64 << 10;
    const PartGeo geos[] = {{4, 2, 8, 0}, {16, 16, 256, 0}};
    double worst = 0;
    for (int k : {31, 51, 127}) {
        const int W = k / 32 + 1;
        const std::pair<uint64_t, uint64_t> sparse{(uint64_t)k, 20000}, dense{4991, 40}, half{(uint64_t)k, 10000};
        const std::vector<std::vector<std::pair<uint64_t, uint64_t>>> streams = {
            {sparse, dense}, {dense, sparse}, {half, dense, half}};
        for (size_t si = 0; si < streams.size(); si++) {
            uint64_t total = 0;
            const std::vector<uint32_t> bk = break_words(streams[si], &total, k);
            const uint64_t n_words = bk.size();
            CHECK(packed_windows_host(bk.data(), n_words, k) == total, "window count of stream %zu at k %d", si, k);
            for (uint64_t hint : {total, (uint64_t)0, 8 * total, total / 8, (uint64_t)1}) {
                // packed_pass's cuts: the first word at or past the cut length whose first symbol is a break
                const uint64_t lim = packed_cut_words(batch_bytes, n_words, hint);
                std::vector<uint64_t> cuts{0};
                while (n_words - cuts.back() > lim) {
                    uint64_t w = cuts.back() + lim;
                    while (w < n_words && !(bk[w] >> 31)) w++;
                    if (w >= n_words) break;
                    cuts.push_back(w);
                }
                cuts.push_back(n_words);
                const size_t nb = cuts.size() - 1;
                std::vector<uint64_t> bw(nb);
                uint64_t sum = 0, maxs = 0;
                double measured = 0;
                for (size_t i = 0; i < nb; i++) {
                    const uint64_t syms = (cuts[i + 1] - cuts[i]) * 32;
                    bw[i] = packed_windows_host(bk.data() + cuts[i], cuts[i + 1] - cuts[i], k);
                    sum += bw[i];
                    maxs = std::max(maxs, syms);
                    measured = std::max(measured, packed_batch_density(bw[i], syms));
                }
                CHECK(sum == total, "no window spans a cut: stream %zu k %d hint %" PRIu64, si, k, hint);
                const double hd = packed_hint_density(n_words, hint);
                const double dens = packed_plan_density(hd, measured);
                for (size_t i = 0; i < nb; i++) {
                    const uint64_t syms = (cuts[i + 1] - cuts[i]) * 32;
                    if (hint == total) worst = std::max(worst, (double)bw[i] / (double)plan_window_bound(syms, hd));
                    for (const PartGeo& g0 : geos) {
                        PartGeo g = g0;
                        g.IW = W;
                        for (const Layout& l : kLayouts)  // (a deferred pass plans every batch at the largest)
                            check_plan("heterogeneous", W, g, l.tight ? maxs : syms, bw[i], dens, l, PlanKnobs{});
                    }
                }
            }
        }
    }
    std::printf("heterogeneous rows: densest batch holds %.2f x the windows the exact hint's density plans for\n", worst);
}

int main() {
    sweep_plans();
    sweep_cuts();
    heterogeneous_rows();
    std::printf("plan_host_check: %ld checks, %ld failed\n", g_checks, g_fails);
    return g_fails ? 1 : 0;
}
