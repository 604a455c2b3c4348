// kc_graph_impl.h -- the de Bruijn graph of the counted full-key table, kernels for one key width W
// (instantiated by kc_graph_w.hip): k_neighbors, the counts of the eight neighbours of given
// k-mers, and k_graph_edges + k_graph_links, one sweep pair that gives every node its eight edge
// bits, its two unitig-link bits and the whole graph's statistics (the definitions:
// include/kc_api.h kc_graph_device).  The reference has no counterpart: its users rebuild a hash
// table from the output text to ask what follows a k-mer.
//
// The table keys are bijective (from_tkey), so a slot gives its canonical k-mer K; from K and
// rc(K), computed once per k-mer, the eight neighbours come from shifts alone (neighbor_tkeys,
// kc_key.h): K[1:] + y is K shifted left one character with y appended, and its reverse complement
// is rc(K) shifted right with 3 - y prepended; the L side is the mirror image.  No neighbour is
// reverse-complemented on its own.  A thread forms and probes one neighbour at a time (W goes up
// to 15 words).
//
// All three kernels only read the table, by the rules of kc_table_read.h: plain loads, every probe
// bounded by BPR buckets.
//
//   k_graph_edges  sweeps the table and, for every node (an occupied slot with lo <= T(c) <= hi),
//                  probes its eight neighbours (table_count_word) and writes one edge byte, bit y =
//                  side R, bit 4 + y = side L, into edges[bucket * S + slot] (0 for every other slot).
//   k_graph_links  a second launch on the same stream: it reads the edge bytes and never writes
//                  them.  For each side of degree 1 of a node it forms that one neighbour again,
//                  probes for its slot (graph_probe_slot), reads the neighbour's edge byte and
//                  applies the link rule; statistics are reduced per workgroup (one atomic per
//                  non-zero field) and the records of a tile of slots are appended behind one
//                  cursor, one atomic per workgroup and tile (block_reserve, kc_block.h), bounded
//                  by the caller's capacity.
//
// The sweeps take one slot per thread: a bucket per thread (as k_join sweeps) serialises the S * 8
// probes of a bucket in one lane.  On a C2 table with every k-mer a node the slot form is faster
// at every width measured (28.7 against 35.2 ms at k = 31, 59.9 / 60.8 at 51, 46.4 / 50.1 at 127);
// the bucket form wins by a tenth where four of ten occupied slots are skipped (T(c) >= 2 at k = 31
// and 51).  DESIGN.md 3a has the figures; -DKC_GRAPH_BUCKET_MAP builds the bucket form.
#pragma once
#include "kc_block.h"
#include "kc_key.h"
#include "kc_table_read.h"

namespace kc {

constexpr int GRAPH_T = BLOCK_T;
constexpr uint64_t GRAPH_BLOCKS = 8192;  // grid-stride: 32 workgroups per CU
#ifdef KC_GRAPH_BUCKET_MAP
constexpr bool GRAPH_BUCKET_MAP = true;
#else
constexpr bool GRAPH_BUCKET_MAP = false;
#endif
// the words of the statistics scratch: the ten of kc_graph_stats, then the record cursor
constexpr int GS_CURSOR = 10;
static_assert(GS_CURSOR + 1 == GRAPH_STAT_WORDS, "kc_internal.h states the scratch's size");

// the slot (bucket * S + slot) of table key t in tv, NO_SLOT when the table does not hold it
template <int W>
DEV uint64_t graph_probe_slot(const TableView& tv, const uint64_t (&t)[W]) {
    return table_probe<W>(tv, t, NO_SLOT, [](uint64_t bucket, const uint64_t*, int sl) {
        return bucket * (BUCKET_WORDS / (W + 1)) + sl;
    });
}

// ---- k_neighbors: counts[8 i + j] = T of neighbour j of key i ------------------------------------
template <int W>
__global__ __launch_bounds__(GRAPH_T) void k_neighbors(TableView tv, int k, int count_mode, int layout,
                                                       const uint64_t* __restrict__ keys, uint64_t n,
                                                       uint32_t* __restrict__ counts) {
    const uint64_t i = (uint64_t)blockIdx.x * GRAPH_T + threadIdx.x;
    if (i >= n) return;
    const RollConst rk = make_roll<W>(k, 0, 0);
    uint64_t q[W], K[W], RC[W];
#pragma unroll
    for (int j = 0; j < W; j++) q[j] = keys[i * W + j];
    // as query_tkey validates, but the orientation stays as given: R and L are the strand's own
    bool ok;
    if (layout == KC_KEYS_TABLE) {
        ok = q[0] != EMPTY;
        from_tkey<W>(q, K);
    } else {
        ok = !(q[0] & ~rk.topmask);  // a bit above 2k - 1
#pragma unroll
        for (int j = 0; j < W; j++) K[j] = q[j];
    }
    revcomp<W>(K, rk, RC);
    uint32_t* out = counts + i * 8;
#pragma unroll 1
    for (int j = 0; j < 8; j++) {
        uint32_t c = 0;
        if (ok) {
            uint64_t t[W];
            neighbor_tkeys<W>(K, RC, j, rk, t);
            bool found;
            const uint64_t cw = table_count_word<W>(tv, t, found);
            if (found) c = tc_of(cw, count_mode);
        }
        out[j] = c;
    }
}

// ---- the sweep of k_graph_edges / k_graph_links --------------------------------------------------
// The table in tiles, a workgroup at a time: f(in, slot, tk, cw, r) for every slot of the tile --
// slot = bucket * S + sl, tk its key words, cw its count word, in = false past the table's end, r <
// GRAPH_RPT the number of the call in this thread's tile -- then tile_end(), which every thread of
// the workgroup reaches together (k_graph_links takes the tile's place in the records there).
// BM: a bucket per thread (a tile is GRAPH_T buckets, f called S times), else a slot per thread and
// GRAPH_ITERS of them in turn (a tile is GRAPH_T * GRAPH_ITERS consecutive slots).
constexpr int GRAPH_ITERS = 8;
constexpr int GRAPH_RPT = 8;  // f calls per thread and tile: max(S, GRAPH_ITERS)
template <int W, bool BM>
constexpr uint64_t graph_tile_items() {
    return BM ? GRAPH_T : GRAPH_T * GRAPH_ITERS;
}
template <int W, bool BM, class F, class G>
DEV void graph_sweep(const TableView& tv, F&& f, G&& tile_end) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    static_assert(S <= GRAPH_RPT && GRAPH_ITERS <= GRAPH_RPT, "a thread's calls of a tile");
    const uint64_t n_items = BM ? tv.nbuckets : tv.nbuckets * S;
    constexpr uint64_t TILE = graph_tile_items<W, BM>();
    for (uint64_t tile0 = (uint64_t)blockIdx.x * TILE; tile0 < n_items; tile0 += (uint64_t)gridDim.x * TILE) {
        if constexpr (BM) {
            const uint64_t it = tile0 + threadIdx.x;
            const bool in = it < n_items;
            uint64_t bw[BUCKET_WORDS];
            if (in) {
                load_bucket(tv.buckets + it * BUCKET_WORDS, bw);
            } else {
#pragma unroll
                for (int i = 0; i < BUCKET_WORDS; i++) bw[i] = 0;
            }
#pragma unroll
            for (int sl = 0; sl < S; sl++) {
                uint64_t tk[W];
#pragma unroll
                for (int i = 0; i < W; i++) tk[i] = bw[sl * W + i];
                f(in, it * S + sl, tk, bw[S * W + sl], sl);
            }
        } else {
#pragma unroll 1
            for (int j = 0; j < GRAPH_ITERS; j++) {
                const uint64_t it = tile0 + (uint64_t)j * GRAPH_T + threadIdx.x;
                const bool in = it < n_items;
                const uint64_t bucket = it / S;
                const int sl = (int)(it - bucket * S);
                uint64_t tk[W];
                // past the end slot 0's words, then zeroed: the loads under `if (in)` cost
                // k_unitig_succ<3> and <7> an occupancy step (profiles/table_read_resources.md)
                slot_tkey<W>(tv, in ? it : 0, tk);
#pragma unroll
                for (int i = 0; i < W; i++) tk[i] = in ? tk[i] : 0;
                const uint64_t cw = in ? tv.buckets[bucket * BUCKET_WORDS + S * W + sl] : 0;
                f(in, it, tk, cw, j);
            }
        }
        tile_end();
    }
}

struct GraphArgs {
    TableView tv;
    int k, count_mode;
    uint32_t lo, hi;            // the node range on T(c) (lo >= 1, hi 0 = no upper bound)
    uint8_t* edges;             // nbuckets * S edge bytes
    uint64_t* records;          // W + 1 words per node (nullptr: statistics only)
    uint64_t capacity;          // records that fit
    unsigned long long* stats;  // GRAPH_STAT_WORDS words, zeroed by the caller
};

template <int W>
__global__ __launch_bounds__(GRAPH_T) void k_graph_edges(GraphArgs g) {
    const RollConst rk = make_roll<W>(g.k, 0, 0);
    graph_sweep<W, GRAPH_BUCKET_MAP>(
        g.tv,
        [&](bool in, uint64_t slot, const uint64_t (&tk)[W], uint64_t cw, int) {
            if (!in) return;
            uint32_t e = 0;
            if (tk[0] != EMPTY && in_range(tc_of(cw, g.count_mode), g.lo, g.hi)) {
                uint64_t K[W], RC[W];
                from_tkey<W>(tk, K);
                revcomp<W>(K, rk, RC);
#pragma unroll 1
                for (int i = 0; i < 8; i++) {
                    uint64_t t[W];
                    neighbor_tkeys<W>(K, RC, i, rk, t);
                    bool found;
                    const uint64_t cwn = table_count_word<W>(g.tv, t, found);
                    if (found && in_range(tc_of(cwn, g.count_mode), g.lo, g.hi)) e |= 1u << i;
                }
            }
            g.edges[slot] = (uint8_t)e;
        },
        [] {});
}

template <int W>
__global__ __launch_bounds__(GRAPH_T) void k_graph_links(GraphArgs g) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    const RollConst rk = make_roll<W>(g.k, 0, 0);
    // a tile's records wait here for the tile's place: {slot's T(c) | flags << 32} of call r of thread
    // t at [r][t] (0: no node; only thread t reads it back), so the cursor takes one atomic per
    // tile -- one per wave and iteration, 4 M of them on a C2 table, took 43 ms of one word's
    // ~90 atomics per microsecond
    __shared__ uint64_t s_rec[GRAPH_RPT][GRAPH_T];
    unsigned long long n_nodes = 0, n_edge = 0, n_link = 0, n_iso = 0, n_pal = 0, sd0 = 0, sd1 = 0, sd2 = 0, sd3 = 0,
                       sd4 = 0;
    uint32_t mine = 0;        // this thread's nodes of the tile
    uint64_t first_slot = 0;  // the slot of its call 0, the later ones `step` slots apart
    constexpr uint64_t step = GRAPH_BUCKET_MAP ? 1 : GRAPH_T;
    graph_sweep<W, GRAPH_BUCKET_MAP>(
        g.tv,
        [&](bool in, uint64_t slot, const uint64_t (&tk)[W], uint64_t cw, int r) {
            const uint32_t tc = tc_of(cw, g.count_mode);
            const bool node = in && tk[0] != EMPTY && in_range(tc, g.lo, g.hi);
            uint32_t flags = 0;
            if (node) {
                uint64_t K[W], RC[W];
                from_tkey<W>(tk, K);
                revcomp<W>(K, rk, RC);
                const bool pal = key_eq<W>(K, RC);
                const uint32_t e = g.edges[slot];
                flags = e | KC_GRAPH_NODE;
#pragma unroll 1
                for (int side = 0; side < 2; side++) {
                    const uint32_t nib = (e >> (4 * side)) & 15;
                    const int deg = __popc(nib);
                    sd0 += deg == 0;
                    sd1 += deg == 1;
                    sd2 += deg == 2;
                    sd3 += deg == 3;
                    sd4 += deg == 4;
                    if (deg != 1 || pal) continue;
                    uint64_t t[W];
                    const int ori = neighbor_tkeys<W>(K, RC, 4 * side + (__ffs((int)nib) - 1), rk, t);
                    if (ori == 2 || key_eq<W>(t, tk)) continue;  // the neighbour is a palindrome, or c itself
                    const uint64_t ds = graph_probe_slot<W>(g.tv, t);
                    if (ds == NO_SLOT) continue;  // (an edge's neighbour is in the table)
                    // c sits on the neighbour's side L (R) when it follows (precedes) c as read
                    const int facing = (ori == 0) == (side == 0) ? 1 : 0;
                    if (__popc(((uint32_t)g.edges[ds] >> (4 * facing)) & 15) == 1) flags |= KC_GRAPH_LINK_R << side;
                }
                n_nodes++;
                n_edge += __popc(e);
                n_link += __popc(flags & (KC_GRAPH_LINK_R | KC_GRAPH_LINK_L));
                n_iso += e == 0;
                n_pal += pal;
            }
            if (!g.records) return;
            if (r == 0) first_slot = slot;
            s_rec[r][threadIdx.x] = node ? (uint64_t)tc | (uint64_t)flags << 32 : 0;
            mine += node;
        },
        [&] {
            if (!g.records) return;
            // the tile's place in the records: one atomic per workgroup and tile
            uint64_t idx = block_reserve(mine, g.stats + GS_CURSOR);
            constexpr int RPT = GRAPH_BUCKET_MAP ? S : GRAPH_ITERS;
#pragma unroll 1
            for (int r = 0; r < RPT && mine; r++) {
                const uint64_t v = s_rec[r][threadIdx.x];
                if (!v) continue;
                if (idx < g.capacity) {  // the key again from the table (the tile's lines are in L2)
                    uint64_t tk[W], K[W];
                    slot_tkey<W>(g.tv, first_slot + (uint64_t)r * step, tk);
                    from_tkey<W>(tk, K);
                    uint64_t* o = g.records + idx * (W + 1);
#pragma unroll
                    for (int i = 0; i < W; i++) o[i] = K[i];
                    o[W] = v;
                }
                idx++;
            }
            mine = 0;
            __syncthreads();  // block_reserve's shared words are the next tile's too
        });
    const unsigned long long v[GS_CURSOR] = {n_nodes, n_edge, n_link, n_iso, n_pal, sd0, sd1, sd2, sd3, sd4};
    unsigned long long* dst[GS_CURSOR];
#pragma unroll
    for (int q = 0; q < GS_CURSOR; q++) dst[q] = g.stats + q;
    block_sum_add<GS_CURSOR>(v, dst);
}

template <int W>
hipError_t GraphOps<W>::neighbors(TableView t, int k, int count_mode, int layout, const uint64_t* keys, uint64_t n,
                                  uint32_t* counts, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_neighbors<W>, dim3((unsigned)((n + GRAPH_T - 1) / GRAPH_T)), dim3(GRAPH_T), 0, s, t, k,
                       count_mode, layout, keys, n, counts);
    return hipGetLastError();
}

template <int W>
hipError_t GraphOps<W>::graph(TableView t, int k, int count_mode, uint32_t lo, uint32_t hi, uint8_t* edges,
                              uint64_t* records, uint64_t capacity, unsigned long long* stats, hipStream_t s) {
    if (!t.nbuckets) return hipSuccess;
    const GraphArgs g{t, k, count_mode, lo, hi, edges, records, capacity, stats};
    const uint64_t items = GRAPH_BUCKET_MAP ? t.nbuckets : t.nbuckets * (uint64_t)(BUCKET_WORDS / (W + 1));
    constexpr uint64_t TILE = graph_tile_items<W, GRAPH_BUCKET_MAP>();
    const uint64_t need = (items + TILE - 1) / TILE;
    const unsigned grid = (unsigned)(need < GRAPH_BLOCKS ? need : GRAPH_BLOCKS);
    hipLaunchKernelGGL(k_graph_edges<W>, dim3(grid), dim3(GRAPH_T), 0, s, g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_graph_links<W>, dim3(grid), dim3(GRAPH_T), 0, s, g);
    return hipGetLastError();
}

}  // namespace kc
