// kc_path.hip -- read paths through the compacted graph, the kernels that never touch a key (the
// definitions: include/kc_api.h kc_read_paths_device; the places they read: kc_path_impl.h), and the
// width dispatch of k_path_locate.
//
// A pass is n_pos text positions with a place each.  Position p of sequence [a, e) has a window when
// p + k <= e and its place is not PATH_NOWIN, and is located when that place names a unitig.  From
// its own place and its two neighbours' a position knows everything about itself:
//   run head     located, and p - 1 does not continue it: not in the sequence, not located, another
//                unitig or strand, or a q that is neither one less nor the step n_nodes - 1 -> 0 of a
//                circular unitig (the unitig's node count and its cut's mark are read for that step
//                alone).  It is joined when p - 1 is located all the same.
//   run tail     located, and p + 1 does not continue it.
//   chain head / tail   located, and p - 1 / p + 1 is not; likewise for the stretches of windows.
// Run j of the text is the j-th run head in position order, so the heads are numbered by an ordered
// prefix sum -- no atomic cursor, no sort:
//   k_path_tiles  per tile of PATH_T positions the number of run heads and the last run head, chain
//                 head and window head in it.
//   k_path_scan   one workgroup: the exclusive prefix over the tiles (sum, and max of the
//                 positions), starting at the run cursor the pass before left, which it moves on.
//   k_path_emit   the flags again, an inclusive scan inside the tile on top of the tile's prefix.
//                 A run TAIL writes the record: the heads up to it number it, the last run head at
//                 or before it is its first window, so windows = tail - head + 1 and nothing is
//                 walked; rec[start] names the unitig.  Two 16-byte stores per record.  The tails add
//                 the sequence's sums (one atomic per run, chain and stretch of windows, not per
//                 window) and the position a sequence starts at writes its first_run, for the empty
//                 sequences before it too.
//   k_path_finish a thread per sequence of the pass: seqs and threaded.
#include "kc_block.h"
#include "kc_common.h"
#include "kc_internal.h"

namespace kc {

static_assert(PATH_T == BLOCK_T, "the path kernels reduce with block_sum_add");
static_assert(sizeof(kc_path_run) == 32 && sizeof(kc_path_seq) == 32, "include/kc_api.h states these sizes");

// the sequence of position p <= n_pos: the last i in [i0, i1) with off[i] - base <= p (i1 > i0)
DEV uint64_t path_seq_of(const PathPass& P, uint64_t p) {
    uint64_t lo = P.i0, hi = P.i1;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (P.off[mid] - P.base <= p) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct PathPos {
    bool win, loc;
    uint32_t x, y;
};
// position p of a sequence that ends at e (both counted from the pass's first byte)
DEV PathPos path_pos(const PathPass& P, uint64_t p, uint64_t e) {
    PathPos r{false, false, 0, 0};
    if (p + (uint64_t)P.k > e) return r;  // (e <= n_pos: place[p] exists)
    const uint2 v = P.place[p];
    r.win = v.x != PATH_NOWIN;
    r.loc = r.win && v.x != PATH_NONE;
    r.x = v.x;
    r.y = v.y;
    return r;
}
// b, one position after a, continues a's run
DEV bool path_cont(const PathPos& a, const PathPos& b, const UnitigBufs& u, const UnitigState* __restrict__ F) {
    if (!a.loc || !b.loc || a.x != b.x || ((a.y ^ b.y) >> 31)) return false;
    const uint32_t qa = a.y & 0x7FFFFFFFu, qb = b.y & 0x7FFFFFFFu;
    if (qb == qa + 1) return true;
    if (qb != 0) return false;
    // round the circle: from the last node to the first (a circle's leader carries the cut's mark)
    return (uint64_t)qa + 1 == u.off[2 * (uint64_t)a.x + 1] && F[2 * (uint64_t)a.x + 1].mn == UNITIG_CIRC;
}

struct PathFlags {
    uint64_t s, a, e;  // the sequence and its bytes [a, e) in the pass
    PathPos cur;
    bool head, chain_head, win_head, tail, chain_tail, win_tail;
};
DEV PathFlags path_flags(const PathPass& P, const UnitigBufs& u, const UnitigState* __restrict__ F, uint64_t p) {
    PathFlags f;
    f.s = path_seq_of(P, p);
    f.a = P.off[f.s] - P.base;
    f.e = P.off[f.s + 1] - P.base;
    f.cur = path_pos(P, p, f.e);
    const PathPos none{false, false, 0, 0};
    const PathPos prev = p > f.a ? path_pos(P, p - 1, f.e) : none;
    const PathPos next = path_pos(P, p + 1, f.e);
    f.head = f.cur.loc && !path_cont(prev, f.cur, u, F);
    f.chain_head = f.cur.loc && !prev.loc;
    f.win_head = f.cur.win && !prev.win;
    f.tail = f.cur.loc && !path_cont(f.cur, next, u, F);
    f.chain_tail = f.cur.loc && !next.loc;
    f.win_tail = f.cur.win && !next.win;
    return f;
}

DEV unsigned long long path_max(unsigned long long a, unsigned long long b) { return a > b ? a : b; }
// a, then b
DEV PathTile path_join(const PathTile& a, const PathTile& b) {
    return PathTile{a.heads + b.heads, path_max(a.run_head, b.run_head), path_max(a.chain_head, b.chain_head),
                    path_max(a.win_head, b.win_head)};
}
// the inclusive scan of v over the workgroup's threads; every thread calls it
DEV PathTile path_scan_incl(PathTile v, PathTile (&s_w)[PATH_T / 64]) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int d = 1; d < 64; d <<= 1) {
        PathTile o;
        o.heads = __shfl_up(v.heads, d, 64);
        o.run_head = __shfl_up(v.run_head, d, 64);
        o.chain_head = __shfl_up(v.chain_head, d, 64);
        o.win_head = __shfl_up(v.win_head, d, 64);
        if (lane >= d) v = path_join(o, v);
    }
    __syncthreads();  // (s_w may still be read from the call before)
    if (lane == 63) s_w[wid] = v;
    __syncthreads();
    for (int w = 0; w < PATH_T / 64; w++)
        if (w < wid) v = path_join(s_w[w], v);
    return v;
}
DEV PathTile path_own(const PathFlags& f, uint64_t p) {
    return PathTile{f.head ? 1ull : 0ull, f.head ? p + 1 : 0, f.chain_head ? p + 1 : 0, f.win_head ? p + 1 : 0};
}

__global__ __launch_bounds__(PATH_T) void k_path_tiles(PathPass P, UnitigBufs u, int j, PathTile* __restrict__ tiles) {
    const UnitigState* __restrict__ F = u.st[u.ctl[UC_SRC + j] & 1];
    const uint64_t p = (uint64_t)blockIdx.x * PATH_T + threadIdx.x;
    PathTile v{0, 0, 0, 0};
    if (p < P.n_pos) v = path_own(path_flags(P, u, F, p), p);
    __shared__ PathTile s_w[PATH_T / 64];
    v = path_scan_incl(v, s_w);
    if (threadIdx.x == PATH_T - 1) tiles[blockIdx.x] = v;
}

__global__ __launch_bounds__(PATH_T) void k_path_scan(PathTile* __restrict__ tiles, uint64_t n_tiles,
                                                      unsigned long long* __restrict__ ctl) {
    // s_incl[0]: what lies before the round, s_incl[1 + thread]: with the thread's tile
    __shared__ PathTile s_w[PATH_T / 64], s_incl[PATH_T + 1];
    if (threadIdx.x == 0) s_incl[0] = PathTile{ctl[PC_RUNS], 0, 0, 0};
    __syncthreads();
    for (uint64_t t0 = 0; t0 < n_tiles; t0 += PATH_T) {
        const uint64_t t = t0 + threadIdx.x;
        PathTile v{0, 0, 0, 0};
        if (t < n_tiles) v = tiles[t];
        v = path_scan_incl(v, s_w);
        s_incl[1 + threadIdx.x] = path_join(s_incl[0], v);
        __syncthreads();
        // what lies before a tile is what the tile before it includes
        if (t < n_tiles) tiles[t] = s_incl[threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) s_incl[0] = s_incl[PATH_T];
        __syncthreads();
    }
    if (threadIdx.x == 0) ctl[PC_RUNS] = s_incl[0].heads;
}

__global__ __launch_bounds__(PATH_T) void k_path_emit(PathPass P, UnitigBufs u, int j, const uint32_t* __restrict__ rec,
                                                      const PathTile* __restrict__ tiles, uint4* __restrict__ runs,
                                                      uint64_t cap_runs, kc_path_seq* __restrict__ seq,
                                                      unsigned long long* __restrict__ ctl) {
    const UnitigState* __restrict__ F = u.st[u.ctl[UC_SRC + j] & 1];
    const uint64_t n_nodes = unitig_nodes(u);
    const uint64_t p = (uint64_t)blockIdx.x * PATH_T + threadIdx.x;
    PathFlags f{};
    PathTile v{0, 0, 0, 0};
    if (p <= P.n_pos) {  // (the position one past the pass has no window: every flag is false)
        f = path_flags(P, u, F, p);
        v = path_own(f, p);
    }
    __shared__ PathTile s_w[PATH_T / 64];
    const PathTile in = path_join(tiles[blockIdx.x], path_scan_incl(v, s_w));
    unsigned long long n_win = 0, n_loc = 0, n_chains = 0;
    if (p <= P.n_pos) {
        if (seq && p == f.a) {  // the sequence starts here, and so do the empty ones before it
            const unsigned long long first = in.heads - v.heads;
            for (uint64_t i = f.s;; i--) {
                seq[i].first_run = first;
                if (i == P.i0 || P.off[i - 1] - P.base != p) break;
            }
        }
        if (f.tail && in.run_head) {
            const uint64_t idx = in.heads - 1, hp = in.run_head - 1;
            if (seq) atomicAdd(&seq[f.s].runs, 1u);
            if (runs && idx < cap_runs) {
                const uint2 h = P.place[hp];
                bool joined = false;
                if (hp > f.a) {
                    const uint32_t bx = P.place[hp - 1].x;
                    joined = bx != PATH_NOWIN && bx != PATH_NONE;
                }
                const uint64_t text_pos = P.base + hp;
                const uint32_t unitig = h.x < n_nodes ? rec[h.x] : KC_NO_UNITIG;
                runs[2 * idx] = make_uint4((uint32_t)text_pos, (uint32_t)(text_pos >> 32), (uint32_t)f.s, (uint32_t)(p - hp + 1));
                runs[2 * idx + 1] = make_uint4(unitig, h.y & 0x7FFFFFFFu, (h.y >> 31) | (joined ? KC_RUN_JOINED : 0u), 0);
            }
        }
        if (f.chain_tail && in.chain_head) {
            const uint32_t len = (uint32_t)(p - (in.chain_head - 1) + 1);
            n_loc = len;
            n_chains = 1;
            if (seq) {
                atomicAdd(&seq[f.s].located, len);
                atomicAdd(&seq[f.s].chains, 1u);
                atomicMax(&seq[f.s].longest_chain, len);
            }
        }
        if (f.win_tail && in.win_head) {
            const uint32_t len = (uint32_t)(p - (in.win_head - 1) + 1);
            n_win = len;
            if (seq) atomicAdd(&seq[f.s].windows, len);
        }
    }
    const unsigned long long sums[3] = {n_win, n_loc, n_chains};
    unsigned long long* const dst[3] = {ctl + PC_WINDOWS, ctl + PC_LOCATED, ctl + PC_CHAINS};
    block_sum_add<3>(sums, dst);
}

__global__ __launch_bounds__(PATH_T) void k_path_finish(const kc_path_seq* __restrict__ seq, uint64_t i0, uint64_t i1,
                                                        unsigned long long* __restrict__ ctl) {
    unsigned long long n_seqs = 0, n_threaded = 0;
    for (uint64_t i = i0 + (uint64_t)blockIdx.x * PATH_T + threadIdx.x; i < i1; i += (uint64_t)gridDim.x * PATH_T) {
        n_seqs++;
        const uint32_t w = seq[i].windows;
        n_threaded += w > 0 && seq[i].longest_chain == w;
    }
    const unsigned long long sums[2] = {n_seqs, n_threaded};
    unsigned long long* const dst[2] = {ctl + PC_SEQS, ctl + PC_THREADED};
    block_sum_add<2>(sums, dst);
}

hipError_t launch_path_runs(PathPass p, UnitigBufs u, int rounds, const uint32_t* rec, PathTile* tiles, void* runs,
                            uint64_t cap_runs, kc_path_seq* seq, unsigned long long* ctl, hipStream_t s) {
    if (p.i1 <= p.i0) return hipSuccess;
    const uint64_t n_tiles = path_tiles(p.n_pos);
    if (n_tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_path_tiles, dim3((unsigned)n_tiles), dim3(PATH_T), 0, s, p, u, 2 * rounds, tiles);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_path_scan, dim3(1), dim3(PATH_T), 0, s, tiles, n_tiles, ctl);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(k_path_emit, dim3((unsigned)n_tiles), dim3(PATH_T), 0, s, p, u, 2 * rounds, rec, tiles,
                       (uint4*)runs, runs ? cap_runs : 0, seq, ctl);
    return hipGetLastError();
}

hipError_t launch_path_finish(const kc_path_seq* seq, uint64_t i0, uint64_t i1, unsigned long long* ctl, hipStream_t s) {
    if (i1 <= i0) return hipSuccess;
    const uint64_t need = (i1 - i0 + PATH_T - 1) / PATH_T;
    hipLaunchKernelGGL(k_path_finish, dim3((unsigned)(need < 4096 ? need : 4096)), dim3(PATH_T), 0, s, seq, i0, i1, ctl);
    return hipGetLastError();
}

// W-dispatch of the locate kernel (kc_path_w.hip, one translation unit per key width)
hipError_t launch_path_locate(TableView t, PackedView sv, UnitigBufs u, int k, uint64_t n_pos, uint64_t n_sym,
                              uint2* place, hipStream_t s) {
    KC_DISPATCH(PathOps, t.W, locate(t, sv, u, k, n_pos, n_sym, place, s));
}

}  // namespace kc
