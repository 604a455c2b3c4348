// kc_path_host.h -- the host arithmetic of the read paths (include/kc_api.h kc_read_paths_device):
// the cut of a text into passes, and the bookkeeping of a GAF line.  No HIP: kc_api_path.cpp and
// kc_cli.cpp include it, and tools/path_host_check.cpp runs it under the sanitizers.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace kc {

// Passes: whole sequences of at most batch_bytes together, one longer sequence a pass of its own,
// at most max_seqs sequences in a pass.  offsets: n_seqs + 1 non-decreasing entries.
struct PathPassCut {
    uint64_t i0, i1;  // the sequences [i0, i1)
};
struct PathPlan {
    std::vector<PathPassCut> passes;
    uint64_t max_len = 0;  // bytes of the longest pass
};
inline PathPlan path_plan(const uint64_t* offsets, uint64_t n_seqs, uint64_t batch_bytes, uint64_t max_seqs = 1ull << 30) {
    PathPlan plan;
    for (uint64_t i = 0; i < n_seqs;) {
        PathPassCut p{i, i + 1};
        while (p.i1 < n_seqs && offsets[p.i1 + 1] - offsets[i] <= batch_bytes && p.i1 - i < max_seqs) p.i1++;
        const uint64_t len = offsets[p.i1] - offsets[i];
        if (len > plan.max_len) plan.max_len = len;
        plan.passes.push_back(p);
        i = p.i1;
    }
    return plan;
}

// One GAF line's path: the segment visits of a chain and the lengths that go with them.  A run of
// `windows` windows from q on a unitig of n_nodes nodes visits it once, a circular one once per lap
// begun: (q + windows - 1) / n_nodes + 1 times.  plen is the sum of the visited segments' lengths
// (n_nodes + k - 1 each) less k - 1 per junction; pstart is the first run's q, and pend - pstart =
// the chain's windows + k - 1.
struct GafPath {
    std::string path;
    uint64_t plen = 0, pstart = 0, pend = 0, windows = 0, visits = 0;
};
inline void gaf_add_run(GafPath& g, uint64_t segment, bool rev, uint64_t q, uint64_t windows, uint64_t n_nodes,
                        bool circular, int k) {
    const uint64_t laps = circular && n_nodes ? (q + windows - 1) / n_nodes + 1 : 1;
    if (!g.visits) g.pstart = q;
    for (uint64_t l = 0; l < laps; l++) {
        g.path += rev ? '<' : '>';
        g.path += std::to_string(segment);
        g.plen += n_nodes + (uint64_t)k - 1;
        if (g.visits) g.plen -= (uint64_t)k - 1;
        g.visits++;
    }
    g.windows += windows;
    g.pend = g.pstart + g.windows + (uint64_t)k - 1;
}

}  // namespace kc
