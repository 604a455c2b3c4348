// weak_rule_check.cpp -- the comparison of weak-link removal's rule (csrc/kc_weak_rule.h), the code
// k_weak_verdict runs, in a program of its own against 128-bit integers, for the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o bin/weak_rule_check tools/weak_rule_check.cpp
// (make bin/weak_rule_check; WEAKFLAGS=-DKC_WEAK_MUTANT_64: the check's own mutation check, the
// reference cut to 64 bits -- it must fail).  It touches no device and exits 0 when every check
// holds.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../csrc/kc_weak_rule.h"

typedef unsigned __int128 u128;

// the rule as include/kc_api.h states it; `entries` pairs of (n, count_sum)
static bool reference(uint64_t count_sum, uint64_t n, const uint64_t (*entries)[2], int n_entries, uint32_t ratio) {
    u128 local_n = 0, local_sum = 0;
    for (int i = 0; i < n_entries; i++) local_n += entries[i][0], local_sum += entries[i][1];
    const u128 lhs = (u128)count_sum * local_n * 1000, rhs = (u128)ratio * local_sum * n;
#ifdef KC_WEAK_MUTANT_64
    return (uint64_t)lhs < (uint64_t)rhs;
#else
    return lhs < rhs;
#endif
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static uint64_t rnd() {  // xorshift64*
    rng_state ^= rng_state >> 12, rng_state ^= rng_state << 25, rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1DULL;
}
static uint64_t below(uint64_t bound) { return rnd() % bound; }

int main() {
    using namespace kc;
    unsigned long long checked = 0, failed = 0, wide = 0, flips64 = 0, weak = 0;
    auto one = [&](uint64_t count_sum, uint64_t n, const uint64_t (*entries)[2], int n_entries, uint32_t ratio) {
        WeakLocal loc{0, 0, 0};
        u128 local_n = 0, local_sum = 0;
        for (int i = 0; i < n_entries; i++) {
            weak_local_add(loc, entries[i][0], entries[i][1]);
            local_n += entries[i][0], local_sum += entries[i][1];
        }
        const bool sums_ok = loc.n == (uint64_t)local_n && loc.sum_lo == (uint64_t)local_sum && loc.sum_hi == (uint64_t)(local_sum >> 64);
        const bool want = reference(count_sum, n, entries, n_entries, ratio), got = weak_below(count_sum, n, loc, ratio);
        const u128 lhs = (u128)count_sum * local_n * 1000, rhs = (u128)ratio * local_sum * n;
        wide += (lhs >> 64) != 0 || (rhs >> 64) != 0;
        flips64 += (lhs < rhs) != ((uint64_t)lhs < (uint64_t)rhs);
        weak += want;
        checked++;
        if (!sums_ok || want != got) {
            failed++;
            if (failed <= 5)
                std::printf("FAIL count_sum %llu n %llu entries %d ratio %u: want %d got %d sums %d\n",
                            (unsigned long long)count_sum, (unsigned long long)n, n_entries, ratio, want, got, sums_ok);
        }
    };
    // the largest values the header allows: T(c) < 2^32, ids < 2^30, eight entries of one unitig each
    const uint64_t N_MAX = (1ULL << 30) - 1, T_MAX = 0xFFFFFFFFULL, S_MAX = N_MAX * T_MAX;
    {
        uint64_t e[8][2];
        for (auto& x : e) x[0] = N_MAX, x[1] = S_MAX;
        for (uint32_t ratio : {1u, 200u, 999u, 1000u}) {
            one(S_MAX, N_MAX, e, 8, ratio);
            one(N_MAX, N_MAX, e, 8, ratio);
            one(S_MAX, 1, e, 8, ratio);
            one(1, N_MAX, e, 8, ratio);
        }
    }
    // equal sides: strict.  mean 2 among neighbours of mean 10 at 200 per mille, at every scale
    for (int shift = 0; shift < 28; shift++) {
        const uint64_t n = 1ULL << shift, t = T_MAX / 10;
        const uint64_t e[2][2] = {{3 * n, 3 * n * 10 * t}, {5 * n, 5 * n * 10 * t}};
        one(n * 2 * t, n, e, 2, 200);      // equal: not below
        one(n * 2 * t, n, e, 2, 201);      // below
        one(n * 2 * t - 1, n, e, 2, 200);  // one count less: below
        one(n * 2 * t + 1, n, e, 2, 201);
    }
    // sides that differ by little, far above 2^64: count_sum(U) just around ratio / 1000 of the local mean
    for (int i = 0; i < 200000; i++) {
        const int n_entries = 1 + (int)below(8);
        uint64_t e[8][2];
        const uint64_t scale = 1ULL << below(30);
        u128 local_n = 0, local_sum = 0;
        for (int j = 0; j < n_entries; j++) {
            e[j][0] = 1 + below(scale);
            e[j][1] = e[j][0] * (1 + below(i % 2 ? T_MAX : 65536));
            local_n += e[j][0], local_sum += e[j][1];
        }
        const uint64_t n = 1 + below(scale);
        const uint32_t ratio = 1 + (uint32_t)below(1000);
        // the count_sum at which the two sides meet, and its neighbours
        const u128 meet = (u128)ratio * local_sum * n / (local_n * 1000);
        const uint64_t cap = n * T_MAX;
        for (int d = -2; d <= 2; d++) {
            const u128 c = meet + (u128)(d + 2) < 2 ? 0 : meet + (u128)(d + 2) - 2;
            one(c > cap ? cap : (uint64_t)c, n, e, n_entries, ratio);
        }
        one(below(cap) + 1, n, e, n_entries, ratio);
    }
    std::printf("weak_rule_check: %llu checked, %llu with a side above 2^64, %llu where 64 bits give the other verdict, "
                "%llu weak, %llu failed\n", checked, wide, flips64, weak, failed);
    // the sweep must reach what the tests on a device cannot
    if (!wide || !flips64 || !weak || weak == checked) {
        std::printf("FAIL the sweep does not cover both verdicts above 2^64\n");
        return 1;
    }
    return failed ? 1 : 0;
}
