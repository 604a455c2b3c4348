// kc_unitig_impl.h -- the unitigs of the counted table's de Bruijn graph, the kernels that touch a
// key, for one key width W (instantiated by kc_unitig_w.hip; the definitions: include/kc_api.h
// kc_unitigs_device; the ranking between them: kc_unitig.hip).
//
//   k_graph_edges    (kc_graph_impl.h, as it is) the edge byte of every slot.
//   k_unitig_number  sweeps the table and gives every node a dense id behind one cursor, one atomic
//                    per workgroup and tile as k_graph_links takes its records' places: id_of_slot
//                    (UNITIG_NO_ID for every other slot), tc[id] = T(c), slot_of[id].
//   k_unitig_succ    a second sweep (a partner's tile may be numbered later, so its id is only known
//                    now): the link rule of k_graph_links for both sides of a node, and for the state
//                    (id, side) its successor (partner's id, the other side of the facing side) or
//                    UNITIG_END, and its first UnitigState.  A partner id at or above the node count
//                    becomes UNITIG_END here, so no later kernel follows a wild pointer.
//   k_unitig_emit    every node rebuilds its k-mer from its slot and writes the last base of the
//                    strand it is read on at offset + k - 1 + position; the node at position 0 writes
//                    all k.  A unitig whose bases do not fit has UNITIG_NO_OFF for an offset.
//   k_unitig_edges   (kc_unitig_graph* only) the edges between unitigs: every edge bit of a unitig
//                    end, the neighbour probed for its slot and mapped to its unitig's record.
//
// The table is only read (kc_table_read.h), every probe bounded by BPR; every store index is a
// cursor value below `bound`, an id below the node count, or an offset k_unitig_heads bounded.
#pragma once
#include "kc_graph_impl.h"

namespace kc {

struct UnitigArgs {
    TableView tv;
    int k, count_mode;
    uint32_t lo, hi;
    UnitigBufs u;
};

// the ASCII base of the code in the two lowest bits
DEV uint8_t unitig_base(uint64_t c) { return (uint8_t)(0x54474341u >> (8 * ((uint32_t)c & 3))); }

template <int W>
__global__ __launch_bounds__(GRAPH_T) void k_unitig_number(UnitigArgs g) {
    __shared__ uint32_t s_tc[GRAPH_RPT][GRAPH_T];  // T(c) of call r of thread t, 0: no node
    uint32_t mine = 0;
    uint64_t first_slot = 0;
    constexpr uint64_t step = GRAPH_BUCKET_MAP ? 1 : GRAPH_T;
    constexpr int S = BUCKET_WORDS / (W + 1);
    graph_sweep<W, GRAPH_BUCKET_MAP>(
        g.tv,
        [&](bool in, uint64_t slot, const uint64_t (&tk)[W], uint64_t cw, int r) {
            const uint32_t tc = tc_of(cw, g.count_mode);
            const bool node = in && tk[0] != EMPTY && in_range(tc, g.lo, g.hi);
            if (r == 0) first_slot = slot;
            s_tc[r][threadIdx.x] = node ? tc : 0;  // (a node's T(c) is at least lo >= 1)
            mine += node;
            if (in && !node) g.u.id_of_slot[slot] = UNITIG_NO_ID;
        },
        [&] {
            uint64_t id = block_reserve(mine, g.u.ctl + UC_NODES);
            constexpr int RPT = GRAPH_BUCKET_MAP ? S : GRAPH_ITERS;
#pragma unroll 1
            for (int r = 0; r < RPT && mine; r++) {
                const uint32_t tc = s_tc[r][threadIdx.x];
                if (!tc) continue;
                const uint64_t slot = first_slot + (uint64_t)r * step;
                const bool fits = id < g.u.bound;
                g.u.id_of_slot[slot] = fits ? (uint32_t)id : UNITIG_NO_ID;
                if (fits) {
                    g.u.tc[id] = tc;
                    g.u.slot_of[id] = slot;
                }
                id++;
            }
            mine = 0;
            __syncthreads();  // block_reserve's shared words are the next tile's too
        });
}

template <int W>
__global__ __launch_bounds__(GRAPH_T) void k_unitig_succ(UnitigArgs g) {
    const RollConst rk = make_roll<W>(g.k, 0, 0);
    const uint64_t n_nodes = unitig_nodes(g.u);
    graph_sweep<W, GRAPH_BUCKET_MAP>(
        g.tv,
        [&](bool in, uint64_t slot, const uint64_t (&tk)[W], uint64_t cw, int) {
            const uint32_t tc = tc_of(cw, g.count_mode);
            if (!(in && tk[0] != EMPTY && in_range(tc, g.lo, g.hi))) return;
            const uint32_t id = g.u.id_of_slot[slot];
            if (id >= n_nodes) return;
            uint64_t K[W], RC[W];
            from_tkey<W>(tk, K);
            revcomp<W>(K, rk, RC);
            const bool pal = key_eq<W>(K, RC);
            const uint32_t e = g.u.edges[slot];
#pragma unroll 1
            for (int side = 0; side < 2; side++) {
                const uint32_t nib = (e >> (4 * side)) & 15;
                uint32_t nx = UNITIG_END;
                if (__popc(nib) == 1 && !pal) {  // the link rule, as k_graph_links has it
                    uint64_t t[W];
                    const int ori = neighbor_tkeys<W>(K, RC, 4 * side + (__ffs((int)nib) - 1), rk, t);
                    if (ori != 2 && !key_eq<W>(t, tk)) {
                        const uint64_t ds = graph_probe_slot<W>(g.tv, t);
                        if (ds != NO_SLOT) {
                            const int facing = (ori == 0) == (side == 0) ? 1 : 0;
                            if (__popc(((uint32_t)g.u.edges[ds] >> (4 * facing)) & 15) == 1) {
                                const uint32_t pid = g.u.id_of_slot[ds];
                                if (pid < n_nodes && pid != id) nx = 2 * pid + (uint32_t)(1 - facing);
                            }
                        }
                    }
                }
                const uint32_t x = 2 * id + (uint32_t)side;
                g.u.succ[x] = nx;
                UnitigState st;
                st.mn = id;
                st.stamp = 0;
                if (nx == UNITIG_END) {
                    st.nxt = x | UNITIG_DONE;
                    st.dist = 0;
                    st.sum = 0;
                    g.u.st[1][x] = st;  // an end is final from the start: both buffers hold it
                } else {
                    st.nxt = nx;
                    st.dist = 1;
                    st.sum = g.u.tc[nx >> 1];
                }
                g.u.st[0][x] = st;
            }
        },
        [] {});
}

template <int W>
__global__ __launch_bounds__(GRAPH_T) void k_unitig_emit(TableView tv, int k, UnitigBufs u, uint8_t* __restrict__ bases) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    const RollConst rk = make_roll<W>(k, 0, 0);
    const uint64_t n_nodes = unitig_nodes(u), n_slots = tv.nbuckets * S;
    for (uint64_t i = (uint64_t)blockIdx.x * GRAPH_T + threadIdx.x; i < n_nodes; i += (uint64_t)gridDim.x * GRAPH_T) {
        const uint32_t st = u.start[i];
        if (st >= n_nodes) continue;
        const uint64_t off = u.off[2 * (uint64_t)st];
        if (off == UNITIG_NO_OFF) continue;
        const uint64_t slot = u.slot_of[i];
        if (slot >= n_slots) continue;
        const uint32_t p = u.pos[i], pos = p & 0x7FFFFFFFu;
        if (pos >= u.off[2 * (uint64_t)st + 1]) continue;  // (past the length the offset was bounded with)
        uint64_t tk[W], K[W], X[W];
        slot_tkey<W>(tv, slot, tk);
        from_tkey<W>(tk, K);
        if (p >> 31) {
            revcomp<W>(K, rk, X);
        } else {
#pragma unroll
            for (int j = 0; j < W; j++) X[j] = K[j];
        }
        uint8_t* out = bases + off;
        if (pos) {
            out[(uint64_t)k - 1 + pos] = unitig_base(X[W - 1]);
            continue;
        }
        // character j of the k-mer: bits 2 (k - 1 - j) and up of the 64 W-bit key
#pragma unroll
        for (int wi = 0; wi < W; wi++) {
            const uint64_t w = X[wi];
            const int j0 = k - 1 - 32 * (W - 1 - wi);  // the character in the word's lowest two bits
#pragma unroll 1
            for (int t = 0; t < 32; t++)
                if (j0 - t >= 0) out[j0 - t] = unitig_base(w >> (2 * t));
        }
    }
}

// The edges between unitigs.  A unitig end is a state without a successor (a circle's states all
// have one); the edge bits of the node's side there are the edges, side L of a palindromic node
// aside (its neighbours are side R's).  A tile of GRAPH_T node ids at a time: the count from the
// edge byte alone, the tile's place behind the cursor UC_EDGES with one atomic, and -- only with
// `out` -- one probe per edge for the neighbour's slot, then slot -> id -> start -> record index.
// from_rev: the end's side differs from the one the node is left through as its unitig reads it;
// to_rev: the facing side is the one the neighbour is left through as its unitig reads it.  A
// neighbour the table lacks, or an id or start at or above the node count, cannot be on a table
// that is only read: the record then says UNITIG_NO_ID instead of following it.
template <int W>
__global__ __launch_bounds__(GRAPH_T) void k_unitig_edges(TableView tv, int k, UnitigBufs u, const uint32_t* __restrict__ rec,
                                                          uint4* __restrict__ out, uint64_t cap) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    const RollConst rk = make_roll<W>(k, 0, 0);
    const uint64_t n_nodes = unitig_nodes(u), n_slots = tv.nbuckets * S;
    unsigned long long dead = 0;
    const uint64_t tiles = (n_nodes + GRAPH_T - 1) / GRAPH_T;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t i = tile * GRAPH_T + threadIdx.x;
        uint32_t e = 0;  // the edge bits of this node's unitig ends
        uint64_t slot = NO_SLOT;
        if (i < n_nodes && (slot = u.slot_of[i]) < n_slots) {
            const bool end_r = u.succ[2 * i] == UNITIG_END;
            bool end_l = u.succ[2 * i + 1] == UNITIG_END;
            if (end_l && !(k & 1)) {  // a palindrome (even k only) has no link, so both its sides end
                uint64_t tk[W], K[W], RC[W];
                slot_tkey<W>(tv, slot, tk);
                from_tkey<W>(tk, K);
                revcomp<W>(K, rk, RC);
                if (key_eq<W>(K, RC)) end_l = false;
            }
            const uint32_t eb = u.edges[slot];
            e = (end_r ? eb & 0x0Fu : 0) | (end_l ? eb & 0xF0u : 0);
            dead += (end_r && !(eb & 0x0Fu)) + (end_l && !(eb & 0xF0u));
        }
        const uint32_t mine = (uint32_t)__popc(e);
        uint64_t idx = block_reserve(mine, u.ctl + UC_EDGES);
        if (out && e && idx < cap) {
            uint64_t K[W], RC[W];
            {
                uint64_t tk[W];
                slot_tkey<W>(tv, slot, tk);
                from_tkey<W>(tk, K);
            }
            revcomp<W>(K, rk, RC);
            const bool pal = key_eq<W>(K, RC);
            const uint32_t st = u.start[i], rev = u.pos[i] >> 31;
            const uint32_t from = st < n_nodes ? rec[st] : UNITIG_NO_ID;
#pragma unroll 1
            for (; e && idx < cap; e &= e - 1, idx++) {
                const int b = __ffs((int)e) - 1, side = b >> 2;
                uint64_t t[W];
                const int ori = neighbor_tkeys<W>(K, RC, b, rk, t);
                const uint32_t facing = (ori == 0) == (side == 0) ? 1 : 0;
                const uint64_t ds = graph_probe_slot<W>(tv, t);
                uint32_t to = UNITIG_NO_ID, to_rev = 0;
                if (ds != NO_SLOT) {
                    const uint32_t did = u.id_of_slot[ds];
                    if (did < n_nodes) {
                        const uint32_t sd = u.start[did];
                        if (sd < n_nodes) to = rec[sd];
                        to_rev = ori == 2 ? 0 : (1 - facing) ^ (u.pos[did] >> 31);
                    }
                }
                const uint32_t from_rev = pal ? 0 : (uint32_t)side ^ rev;
                out[idx] = make_uint4(from, to, from_rev | to_rev << 1, 0);  // KC_EDGE_FROM_REV, KC_EDGE_TO_REV
            }
        }
        __syncthreads();  // block_reserve's shared words are the next tile's too
    }
    const unsigned long long v[1] = {dead};
    unsigned long long* const dst[1] = {u.ctl + UC_DEAD};
    block_sum_add<1>(v, dst);
}

template <int W>
hipError_t UnitigOps<W>::succ(TableView t, int k, int count_mode, uint32_t lo, uint32_t hi, UnitigBufs u, hipStream_t s) {
    if (!t.nbuckets) return hipSuccess;
    const GraphArgs ga{t, k, count_mode, lo, hi, u.edges, nullptr, 0, nullptr};
    const UnitigArgs g{t, k, count_mode, lo, hi, u};
    const uint64_t items = GRAPH_BUCKET_MAP ? t.nbuckets : t.nbuckets * (uint64_t)(BUCKET_WORDS / (W + 1));
    constexpr uint64_t TILE = graph_tile_items<W, GRAPH_BUCKET_MAP>();
    const uint64_t need = (items + TILE - 1) / TILE;
    const unsigned grid = (unsigned)(need < GRAPH_BLOCKS ? need : GRAPH_BLOCKS);
    hipLaunchKernelGGL(k_graph_edges<W>, dim3(grid), dim3(GRAPH_T), 0, s, ga);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_unitig_number<W>, dim3(grid), dim3(GRAPH_T), 0, s, g);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_unitig_succ<W>, dim3(grid), dim3(GRAPH_T), 0, s, g);
    return hipGetLastError();
}

template <int W>
hipError_t UnitigOps<W>::emit(TableView t, int k, UnitigBufs u, uint8_t* bases, hipStream_t s) {
    if (!t.nbuckets || !bases) return hipSuccess;
    const uint64_t need = (u.bound + GRAPH_T - 1) / GRAPH_T;
    const unsigned grid = (unsigned)(need < GRAPH_BLOCKS ? (need ? need : 1) : GRAPH_BLOCKS);
    hipLaunchKernelGGL(k_unitig_emit<W>, dim3(grid), dim3(GRAPH_T), 0, s, t, k, u, bases);
    return hipGetLastError();
}

template <int W>
hipError_t UnitigOps<W>::edges(TableView t, int k, UnitigBufs u, const uint32_t* rec, void* out, uint64_t cap, hipStream_t s) {
    if (!t.nbuckets) return hipSuccess;
    const uint64_t need = (u.bound + GRAPH_T - 1) / GRAPH_T;
    const unsigned grid = (unsigned)(need < GRAPH_BLOCKS ? (need ? need : 1) : GRAPH_BLOCKS);
    hipLaunchKernelGGL(k_unitig_edges<W>, dim3(grid), dim3(GRAPH_T), 0, s, t, k, u, rec, (uint4*)(rec ? out : nullptr),
                       out ? cap : 0);
    return hipGetLastError();
}

}  // namespace kc
