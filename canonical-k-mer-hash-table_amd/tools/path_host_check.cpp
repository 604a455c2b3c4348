// path_host_check.cpp -- the host arithmetic of the read paths (csrc/kc_path_host.h) under the
// sanitizers, on the CPU: the cut of a text into passes against its rules stated one by one, and a
// GAF line's lengths against the walk's string built base by base.
//   make bin/path_host_check && bin/path_host_check
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../csrc/kc_path_host.h"

using namespace kc;

static int fails = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            fails++;                                                       \
        }                                                                  \
    } while (0)

static void check_plan(const std::vector<uint64_t>& off, uint64_t batch, uint64_t max_seqs) {
    const uint64_t n = off.size() - 1;
    const PathPlan plan = path_plan(off.data(), n, batch, max_seqs);
    uint64_t next = 0, longest = 0;
    for (size_t j = 0; j < plan.passes.size(); j++) {
        const PathPassCut& p = plan.passes[j];
        CHECK(p.i0 == next && p.i1 > p.i0 && p.i1 <= n);  // the passes tile the sequences, none is empty
        const uint64_t len = off[p.i1] - off[p.i0];
        CHECK(len <= batch || p.i1 == p.i0 + 1);  // a pass above the batch is one sequence
        CHECK(p.i1 - p.i0 <= max_seqs);
        // greedy: the next sequence would not have fitted
        if (p.i1 < n) CHECK(off[p.i1 + 1] - off[p.i0] > batch || p.i1 - p.i0 == max_seqs);
        longest = len > longest ? len : longest;
        next = p.i1;
    }
    CHECK(next == n && plan.max_len == longest);
    CHECK(n != 0 || plan.passes.empty());
}

int main() {
    std::mt19937_64 rng(1);
    // ---- the passes
    check_plan({0}, 100, 8);
    check_plan({0, 0, 0, 0}, 100, 8);
    check_plan({5, 5, 300, 300, 310}, 100, 8);
    check_plan({0, 100, 200, 201}, 100, 8);
    check_plan({0, ~0ULL >> 1}, 1, 1);
    for (int t = 0; t < 2000; t++) {
        std::vector<uint64_t> off{rng() % 7};
        const int n = (int)(rng() % 40);
        for (int i = 0; i < n; i++) off.push_back(off.back() + (rng() % 4 ? rng() % 60 : rng() % 400 ? 0 : rng() % 3000));
        check_plan(off, 1 + rng() % 500, 1 + rng() % 9);
    }
    // ---- a GAF line: segments are random strings that overlap by k - 1 (only their lengths matter here)
    for (int t = 0; t < 2000; t++) {
        const int k = 2 + (int)(rng() % 12);
        auto bases = [&](size_t n) {
            std::string s(n, 'A');
            for (char& c : s) c = "ACGT"[rng() % 4];
            return s;
        };
        GafPath g;
        std::string walk, expect_path;
        uint64_t windows = 0, first_q = 0;
        const int n_runs = 1 + (int)(rng() % 5);
        const bool circle = rng() % 4 == 0;  // a chain on a circle is one run
        for (int r = 0; r < (circle ? 1 : n_runs); r++) {
            const uint64_t n_nodes = 1 + rng() % 20, seg = rng() % 1000;
            const bool rev = rng() & 1;
            std::string s = bases(n_nodes + k - 1);
            // a joined run starts at 0 and the run before it ends at its unitig's end; a circle's goes round
            const uint64_t q = r == 0 ? rng() % n_nodes : 0;
            const uint64_t w = circle ? 1 + rng() % (4 * n_nodes) : (r + 1 < n_runs ? n_nodes - q : 1 + rng() % (n_nodes - q));
            if (r == 0) first_q = q;
            if (r) s.replace(0, k - 1, walk.substr(walk.size() - (k - 1)));  // the segments overlap by k - 1
            const uint64_t laps = circle ? (q + w - 1) / n_nodes + 1 : 1;
            for (uint64_t l = 0; l < laps; l++) {
                walk += walk.empty() ? s : s.substr(k - 1);
                expect_path += (rev ? "<" : ">") + std::to_string(seg);
            }
            gaf_add_run(g, seg, rev, q, w, n_nodes, circle, k);
            windows += w;
        }
        CHECK(g.path == expect_path && g.plen == walk.size() && g.pstart == first_q);
        CHECK(g.windows == windows && g.pend == first_q + windows + k - 1 && g.pend <= g.plen);
    }
    if (fails) {
        std::fprintf(stderr, "path_host_check: %d checks failed\n", fails);
        return 1;
    }
    std::puts("path_host_check: OK");
    return 0;
}
