// kc_unitig.hip -- the unitigs of the counted table's de Bruijn graph, the kernels that never touch a
// key (the definitions: include/kc_api.h kc_unitigs_device; the sweeps before and the bases after:
// kc_unitig_impl.h), and the width dispatch of those.
//
// A unitig is a chain of unknown length, so nothing here walks one: the directed states (node id,
// exit side) form disjoint paths and cycles under `succ`, and list ranking by pointer jumping
// (Wyllie) gives every state the end of its path in log2(longest path) rounds.
//
//   k_unitig_jump   one round: dist[x] += dist[nxt[x]], sum likewise, mn = min, nxt[x] = nxt[nxt[x]],
//                   read from one buffer and written to the other (in place, y's triple is read while
//                   y's thread rewrites it).  A state that reads a DONE state is DONE itself: it
//                   points at the end.  A DONE state is copied across by the next launch (its stamp
//                   says which that is) and then costs one coalesced read a round.  The host enqueues
//                   a fixed number of launches; launch j returns at once when the round before moved
//                   no state, or when 2^round passes the number of states that can be on one path,
//                   and hands the source buffer's index on (UC_SRC + j + 1).  No host readback.
//   k_unitig_cycles_count / _cut   states the first ranking left not DONE lie on cycles, and their mn
//                   is the least node id of the circle: its leader m.  The cut makes (m, L) and the
//                   state whose successor is (m, R) ends and starts every other cycle state again
//                   from succ; the same jump launches rank them (all return at once when the count
//                   is zero).  DONE states are copied across first, so both buffers agree.
//   k_unitig_heads  node c has (end a, dR, sumR) from its R state and (end b, dL, sumL) from its L
//                   state: n = dR + dL + 1, count_sum = sumR + sumL + T(c), the start is the end node
//                   with the smaller id, c is read forward when that is the one through L, and its
//                   position is its distance to the start.  The node at position 0 takes a record
//                   index and a base offset (two atomics per workgroup and tile), writes the record
//                   if it fits and leaves the offset, bounded by cap_bases, at off[2 start], and,
//                   for the edges between unitigs (k_unitig_edges), the record index at rec[start].
//   k_unitig_verdict  (kc_clean* only, after the heads) the node at position 0 again, with n and
//                   count_sum from its two states as above and the two end states a and b themselves:
//                   the unitig is open when succ of both is UNITIG_END (a cut circle's ends have
//                   successors), the degree of an end is the popcount of the nibble of its exit side
//                   in its node's edge byte, and the rule of include/kc_api.h kc_clean_device gives
//                   the verdict byte at its id.  Coalesced: the states, pos; scattered, twice per
//                   unitig: succ, slot_of and the edge byte of an end.
#include "kc_block.h"
#include "kc_common.h"
#include "kc_internal.h"

namespace kc {

constexpr int UT = 256;
static_assert(UT == BLOCK_T, "k_unitig_verdict reduces with block_sum_add");
constexpr uint64_t UNITIG_BLOCKS = 8192;

// phase 0: the first ranking, a path has at most 2 * nodes states; phase 1: the cut circles
__global__ __launch_bounds__(UT) void k_unitig_jump(UnitigBufs u, int j, int round, int phase) {
    const uint64_t n_states = 2 * unitig_nodes(u);
    const unsigned long long lim = phase ? u.ctl[UC_CYCLE] : n_states;
    const uint32_t src = (uint32_t)u.ctl[UC_SRC + j] & 1;
    const bool run = lim && (1ULL << round) <= lim && (round == 0 || u.ctl[UC_MOVED + j - 1]);
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (!run) {
        if (first) u.ctl[UC_SRC + j + 1] = src;
        return;
    }
    if (first) u.ctl[UC_SRC + j + 1] = src ^ 1;
    const UnitigState* __restrict__ S = u.st[src];
    UnitigState* __restrict__ D = u.st[src ^ 1];
    int moved = 0;
    for (uint64_t x = (uint64_t)blockIdx.x * UT + threadIdx.x; x < n_states; x += (uint64_t)gridDim.x * UT) {
        UnitigState a = S[x];
        if (a.nxt & UNITIG_DONE) {
            if (a.stamp == (uint32_t)j) {  // the launch before this one wrote it: the other buffer lacks it
                a.stamp = 0;
                D[x] = a;
            }
            continue;
        }
        if (a.nxt >= n_states) continue;  // (succ is bounded where it is produced)
        const UnitigState b = S[a.nxt];
        a.dist += b.dist;
        a.sum += b.sum;
        a.mn = a.mn < b.mn ? a.mn : b.mn;
        a.nxt = b.nxt;  // with its DONE bit: then b.nxt is the end
        if (a.nxt & UNITIG_DONE) {
            a.stamp = (uint32_t)j + 1;
        } else {
            moved = 1;
        }
        D[x] = a;
    }
    if (__syncthreads_or(moved) && threadIdx.x == 0) u.ctl[UC_MOVED + j] = 1;
}

__global__ __launch_bounds__(UT) void k_unitig_cycles_count(UnitigBufs u, int j) {
    const uint64_t n_states = 2 * unitig_nodes(u);
    const UnitigState* __restrict__ S = u.st[u.ctl[UC_SRC + j] & 1];
    unsigned long long n = 0;
    for (uint64_t x = (uint64_t)blockIdx.x * UT + threadIdx.x; x < n_states; x += (uint64_t)gridDim.x * UT)
        n += !(S[x].nxt & UNITIG_DONE);
    for (int m = 32; m >= 1; m >>= 1) n += __shfl_xor(n, m, 64);
    __shared__ unsigned long long s_n[UT / 64];
    if ((threadIdx.x & 63) == 0) s_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < UT / 64; w++) t += s_n[w];
        if (t) atomicAdd(u.ctl + UC_CYCLE, t);
    }
}

__global__ __launch_bounds__(UT) void k_unitig_cycles_cut(UnitigBufs u, int j) {
    if (!u.ctl[UC_CYCLE]) return;
    const uint64_t n_nodes = unitig_nodes(u), n_states = 2 * n_nodes;
    const uint32_t src = (uint32_t)u.ctl[UC_SRC + j] & 1;
    UnitigState* F = u.st[src];
    UnitigState* O = u.st[src ^ 1];
    for (uint64_t x = (uint64_t)blockIdx.x * UT + threadIdx.x; x < n_states; x += (uint64_t)gridDim.x * UT) {
        UnitigState a = F[x];
        if (a.nxt & UNITIG_DONE) {
            if (a.stamp) {
                a.stamp = 0;
                F[x] = a;
            }
            O[x] = a;
            continue;
        }
        const uint32_t m = a.mn < n_nodes ? a.mn : (uint32_t)(x >> 1);  // the circle's leader
        const uint32_t nx = u.succ[x];
        a.stamp = 0;
        if (x == 2 * (uint64_t)m + 1 || nx == 2 * m || nx >= n_states) {
            // the leader's side-L link is cut: (m, L) ends here, and so does the state that led to (m, R)
            a.nxt = (uint32_t)x | UNITIG_DONE;
            a.dist = 0;
            a.sum = 0;
            a.mn = x == 2 * (uint64_t)m + 1 ? UNITIG_CIRC : m;
            O[x] = a;
        } else {
            a.nxt = nx;
            a.dist = 1;
            a.sum = u.tc[nx >> 1];
            a.mn = m;
        }
        F[x] = a;
    }
}

// exclusive prefix of v over the workgroup and its total; every thread calls it
DEV uint64_t block_excl_sum(uint64_t v, uint64_t& total, unsigned long long (&s_w)[UT / 64]) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    uint64_t incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = __shfl_up((unsigned long long)incl, d, 64);
        if (lane >= d) incl += o;
    }
    __syncthreads();  // (s_w may still be read from the call before)
    if (lane == 63) s_w[wid] = incl;
    __syncthreads();
    uint64_t before = 0;
    total = 0;
    for (int w = 0; w < UT / 64; w++) {
        if (w < wid) before += s_w[w];
        total += s_w[w];
    }
    return before + incl - v;
}

__global__ __launch_bounds__(UT) void k_unitig_heads(UnitigBufs u, int k, int j, uint64_t* __restrict__ records,
                                                     uint64_t cap_unitigs, uint64_t cap_bases,
                                                     uint32_t* __restrict__ rec) {
    const uint64_t n_nodes = unitig_nodes(u), n_states = 2 * n_nodes;
    const UnitigState* __restrict__ F = u.st[u.ctl[UC_SRC + j] & 1];
    __shared__ unsigned long long s_w[UT / 64], s_rec, s_off;
    unsigned long long n_unitigs = 0, n_circ = 0, n_mine = 0, n_bases = 0, n_max = 0;
    const uint64_t tiles = (n_nodes + UT - 1) / UT;
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t i = tile * UT + threadIdx.x;
        bool head = false, circ = false;
        uint64_t n = 0, sum = 0;
        if (i < n_nodes) {
            const UnitigState r = F[2 * i], l = F[2 * i + 1];
            uint32_t a = r.nxt & ~UNITIG_DONE, b = l.nxt & ~UNITIG_DONE, dR = r.dist, dL = l.dist;
            uint64_t sR = r.sum, sL = l.sum;
            // (every state is DONE after the two rankings; one that is not stands alone)
            if (!(r.nxt & UNITIG_DONE) || a >= n_states) a = (uint32_t)(2 * i), dR = 0, sR = 0;
            if (!(l.nxt & UNITIG_DONE) || b >= n_states) b = (uint32_t)(2 * i + 1), dL = 0, sL = 0;
            const uint32_t ea = a >> 1, eb = b >> 1;
            // the start is the end with the smaller id; c is read forward when that is the end through L
            const bool fwd = eb <= ea;
            const uint32_t start = fwd ? eb : ea, pos = fwd ? dL : dR;
            u.start[i] = start;
            u.pos[i] = pos | (fwd ? 0u : 0x80000000u);
            n_mine++;
            if (pos == 0) {
                head = true;
                n = (uint64_t)dR + dL + 1;
                sum = sR + sL + u.tc[i];
                circ = l.mn == UNITIG_CIRC && fwd;
            }
        }
        const uint64_t len = head ? n + (uint64_t)k - 1 : 0;
        uint64_t heads, bases;
        const uint64_t my_rec = block_excl_sum(head, heads, s_w);
        const uint64_t my_off = block_excl_sum(len, bases, s_w);
        if (threadIdx.x == 0) {  // the tile's place in the records and in the bases
            s_rec = heads ? atomicAdd(u.ctl + UC_REC, (unsigned long long)heads) : 0;
            s_off = bases ? atomicAdd(u.ctl + UC_BASE, (unsigned long long)bases) : 0;
        }
        __syncthreads();
        if (head) {
            const uint64_t idx = s_rec + my_rec, off = s_off + my_off;
            if (records && idx < cap_unitigs) {
                uint64_t* o = records + idx * 4;
                o[0] = off;
                o[1] = n;
                o[2] = sum;
                o[3] = circ ? 1 : 0;  // KC_UNITIG_CIRCULAR
            }
            u.off[2 * i] = off + len <= cap_bases ? off : UNITIG_NO_OFF;
            u.off[2 * i + 1] = n;
            if (rec) rec[i] = (uint32_t)idx;  // (ids, and so records, number below 2^30)
            n_unitigs++;
            n_circ += circ;
            n_bases += len;
            n_max = n > n_max ? n : n_max;
        }
        __syncthreads();  // s_rec and s_off are the next tile's too
    }
    // the workgroup's sums, one atomic per non-zero field
    unsigned long long v[5] = {n_unitigs, n_circ, n_mine, n_bases, n_max};
    __shared__ unsigned long long s_red[5][UT / 64];
#pragma unroll
    for (int q = 0; q < 5; q++) {
        unsigned long long x = v[q];
        for (int m = 32; m >= 1; m >>= 1) {
            const unsigned long long o = __shfl_xor(x, m, 64);
            x = q == 4 ? (o > x ? o : x) : x + o;
        }
        if ((threadIdx.x & 63) == 0) s_red[q][threadIdx.x >> 6] = x;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const int q = threadIdx.x;
        unsigned long long x = 0;
        for (int w = 0; w < UT / 64; w++) x = q == 4 ? (s_red[q][w] > x ? s_red[q][w] : x) : x + s_red[q][w];
        if (x) {
            if (q == 4) atomicMax(u.ctl + UC_STATS + q, x);
            else atomicAdd(u.ctl + UC_STATS + q, x);
        }
    }
}

__global__ __launch_bounds__(UT) void k_unitig_verdict(UnitigBufs u, int j, uint64_t n_slots, CleanRule rule,
                                                       unsigned long long* __restrict__ stats) {
    const uint64_t n_nodes = unitig_nodes(u), n_states = 2 * n_nodes;
    const UnitigState* __restrict__ F = u.st[u.ctl[UC_SRC + j] & 1];
    unsigned long long n_unitigs = 0, n_mine = 0, n_tips = 0, n_tip_nodes = 0, n_iso = 0, n_iso_nodes = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * UT + threadIdx.x; i < n_nodes; i += (uint64_t)gridDim.x * UT) {
        n_mine++;
        const UnitigState r = F[2 * i], l = F[2 * i + 1];
        uint32_t a = r.nxt & ~UNITIG_DONE, b = l.nxt & ~UNITIG_DONE, dR = r.dist, dL = l.dist;
        uint64_t sR = r.sum, sL = l.sum;
        // (as k_unitig_heads: a state that is not DONE stands alone)
        if (!(r.nxt & UNITIG_DONE) || a >= n_states) a = (uint32_t)(2 * i), dR = 0, sR = 0;
        if (!(l.nxt & UNITIG_DONE) || b >= n_states) b = (uint32_t)(2 * i + 1), dL = 0, sL = 0;
        const bool fwd = (b >> 1) <= (a >> 1);
        if ((fwd ? dL : dR) != 0) continue;  // not at position 0
        const uint64_t n = (uint64_t)dR + dL + 1, sum = sR + sL + u.tc[i];
        n_unitigs++;
        uint8_t v = CLEAN_KEEP;
        if (u.succ[a] == UNITIG_END && u.succ[b] == UNITIG_END) {  // open
            const bool dead_a = unitig_end_degree(u, a, n_slots) == 0, dead_b = unitig_end_degree(u, b, n_slots) == 0;
            const bool guard = !rule.max_mean || sum <= (uint64_t)rule.max_mean * n;
            if (dead_a && dead_b) {
                if (rule.iso_max_nodes && n <= rule.iso_max_nodes && guard) v = CLEAN_ISOLATED;
            } else if (dead_a || dead_b) {
                if (rule.tip_max_nodes && n <= rule.tip_max_nodes && guard) v = CLEAN_TIP;
            }
        }
        u.verdict[i] = v;
        n_tips += v == CLEAN_TIP;
        n_tip_nodes += v == CLEAN_TIP ? n : 0;
        n_iso += v == CLEAN_ISOLATED;
        n_iso_nodes += v == CLEAN_ISOLATED ? n : 0;
    }
    // kc_clean_stats' first six words
    const unsigned long long v[6] = {n_unitigs, n_mine, n_tips, n_tip_nodes, n_iso, n_iso_nodes};
    unsigned long long* const dst[6] = {stats, stats ? stats + 1 : nullptr, stats ? stats + 2 : nullptr,
                                        stats ? stats + 3 : nullptr, stats ? stats + 4 : nullptr, stats ? stats + 5 : nullptr};
    block_sum_add<6>(v, dst);
}

static unsigned unitig_grid(uint64_t items) {
    const uint64_t need = (items + UT - 1) / UT;
    return (unsigned)(need < UNITIG_BLOCKS ? (need ? need : 1) : UNITIG_BLOCKS);
}

hipError_t launch_unitig_rank(UnitigBufs u, int rounds, hipStream_t s) {
    if (2 * rounds + 1 > UNITIG_MAX_LAUNCHES) return hipErrorInvalidValue;
    const unsigned grid = unitig_grid(2 * u.bound);
    hipError_t e;
    for (int j = 0; j < 2 * rounds; j++) {
        if (j == rounds) {
            hipLaunchKernelGGL(k_unitig_cycles_count, dim3(grid), dim3(UT), 0, s, u, j);
            if ((e = hipGetLastError()) != hipSuccess) return e;
            hipLaunchKernelGGL(k_unitig_cycles_cut, dim3(grid), dim3(UT), 0, s, u, j);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_unitig_jump, dim3(grid), dim3(UT), 0, s, u, j, j % rounds, j / rounds);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_unitig_heads(UnitigBufs u, int k, int rounds, void* records, uint64_t cap_unitigs, uint64_t cap_bases,
                               uint32_t* rec, hipStream_t s) {
    hipError_t e = hipMemsetAsync(u.ctl + UC_REC, 0, (UC_STATS + 5 - UC_REC) * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_unitig_heads, dim3(unitig_grid(u.bound)), dim3(UT), 0, s, u, k, 2 * rounds, (uint64_t*)records,
                       records ? cap_unitigs : 0, cap_bases, rec);
    return hipGetLastError();
}

hipError_t launch_unitig_verdict(UnitigBufs u, int rounds, uint64_t n_slots, CleanRule rule, unsigned long long* stats,
                                 hipStream_t s) {
    if (!u.verdict) return hipErrorInvalidValue;
    const hipError_t e = hipMemsetAsync(u.verdict, CLEAN_KEEP, u.bound, s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_unitig_verdict, dim3(unitig_grid(u.bound)), dim3(UT), 0, s, u, 2 * rounds, n_slots, rule, stats);
    return hipGetLastError();
}

// W-dispatch of the sweeps and the bases (kc_unitig_w.hip, one translation unit per key width)
hipError_t launch_unitig_succ(TableView t, int k, int count_mode, uint32_t lo, uint32_t hi, UnitigBufs u, hipStream_t s) {
    KC_DISPATCH(UnitigOps, t.W, succ(t, k, count_mode, lo, hi, u, s));
}
hipError_t launch_unitig_emit(TableView t, int k, UnitigBufs u, uint8_t* bases, hipStream_t s) {
    KC_DISPATCH(UnitigOps, t.W, emit(t, k, u, bases, s));
}
hipError_t launch_unitig_edges(TableView t, int k, UnitigBufs u, const uint32_t* rec, void* out, uint64_t cap, hipStream_t s) {
    const hipError_t e = hipMemsetAsync(u.ctl + UC_EDGES, 0, (UC_CDBG_ZERO + 1 - UC_EDGES) * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    KC_DISPATCH(UnitigOps, t.W, edges(t, k, u, rec, out, cap, s));
}
// ... and of the graph cleaning's copy (kc_clean_w.hip)
hipError_t launch_clean(TableView src, TableView dst, UnitigBufs u, DevCounters* ctr, unsigned long long* stats,
                        hipStream_t s) {
    KC_DISPATCH(CleanOps, src.W, copy(src, dst, u, ctr, stats, s));
}

}  // namespace kc
