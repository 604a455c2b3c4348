// kc_path_impl.h -- read paths through the compacted graph, the kernel for one key width W
// (instantiated by kc_path_w.hip; the definitions: include/kc_api.h kc_read_paths_device; the run
// heads, the ordered compaction and the records, which touch no key: kc_path.hip).
//
//   k_path_locate  has the shape of k_seq_counts (kc_seq_impl.h): the text arrives as k_seq_pack's
//                  position-preserving packed stream, a thread takes run_width(W) consecutive window
//                  starts, run_windows extracts the first and rolls the rest, each is made canonical
//                  and mixed into its table key.  Instead of a count the window is probed for its
//                  slot (graph_probe_slot, one thread per key: DESIGN.md 3a measured the cooperative
//                  form slower in this shape), and four gathers follow: slot -> node id, id -> start
//                  and position | strand, start -> the unitig's node count.  rev is the window's
//                  strand xor the node's (0 for a palindrome), q the position counted from the end
//                  the oriented unitig starts at.  The place {start, q | rev << 31} -- or PATH_NONE
//                  for a window that is no node of the range, PATH_NOWIN where no window starts --
//                  is written at the window's start position, run_width(W) places of 8 bytes per
//                  thread, so a wave's stores cover one contiguous range.  The lookups of a thread
//                  are independent of each other.  An id or start at or above the node count, or a
//                  position at or above the unitig's length, is PATH_NONE and never followed.
//
// The table is only read (kc_table_read.h: plain loads, every probe bounded by BPR).
#pragma once
#include "kc_graph_impl.h"

namespace kc {

// place[p], p < n_pos: the place of the window sv[p, p + k), PATH_NOWIN if it holds a break or
// p + k > n_sym.  sv holds seq_pack_words(n_sym) words; n_sym >= k (the launcher answers a shorter
// stream itself).
template <int W>
__global__ __launch_bounds__(256) void k_path_locate(TableView tv, PackedView sv, UnitigBufs u, int k, uint64_t n_pos,
                                                     uint64_t n_sym, uint2* __restrict__ place) {
    constexpr int RW = run_width(W);
    constexpr int S = BUCKET_WORDS / (W + 1);
    const uint64_t g = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t s0 = g * RW;
    if (s0 >= n_pos) return;
    const RollConst rk = make_roll<W>(k, 0, 0);
    const uint64_t n_nodes = unitig_nodes(u), n_slots = tv.nbuckets * S;
    // a thread whose first window already ends past the stream rolls the stream's first run with
    // every window refused (the words it reads exist: n_sym >= k)
    const bool live = s0 + (uint64_t)k - 1 < n_sym;
    const uint64_t r0 = (live ? s0 : 0) + (uint64_t)k - 1;
    const uint64_t t1 = live ? n_sym : 0;
    uint32_t rx[RW], ry[RW];
    run_windows<W, RW>(sv, r0, t1, rk, [&](int j, bool ok, const uint64_t (&fwd)[W], const uint64_t (&rc)[W]) {
        uint64_t key[W], t[W];
        canonical<W>(fwd, rc, key);
        to_tkey<W>(key, t);
        uint32_t x = ok ? PATH_NONE : PATH_NOWIN, y = 0;
        const uint64_t slot = ok ? graph_probe_slot<W>(tv, t) : NO_SLOT;
        if (slot != NO_SLOT && slot < n_slots) {
            const uint32_t id = u.id_of_slot[slot];  // UNITIG_NO_ID for a slot outside the range
            if (id < n_nodes) {
                const uint32_t st = u.start[id], p = u.pos[id];
                if (st < n_nodes) {
                    const uint64_t n = u.off[2 * (uint64_t)st + 1];
                    const uint32_t pos = p & 0x7FFFFFFFu;
                    if (pos < n) {
                        // the window reads as the node does inside S_U when both are read on the
                        // same strand of the canonical k-mer; a palindrome has one reading
                        const bool w_rc = !key_eq<W>(key, fwd), pal = key_eq<W>(fwd, rc);
                        const uint32_t rev = pal ? 0u : (uint32_t)w_rc ^ (p >> 31);
                        x = st;
                        y = (rev ? (uint32_t)(n - 1) - pos : pos) | rev << 31;
                    }
                }
            }
        }
        rx[j] = x;
        ry[j] = y;
    });
    if (s0 + RW <= n_pos) {  // (place is an allocation of the context: 16-byte aligned)
        uint4* o = reinterpret_cast<uint4*>(place + s0);
#pragma unroll
        for (int q = 0; q < RW / 2; q++) o[q] = make_uint4(rx[2 * q], ry[2 * q], rx[2 * q + 1], ry[2 * q + 1]);
    } else {
#pragma unroll
        for (int j = 0; j < RW; j++)
            if (s0 + j < n_pos) place[s0 + j] = make_uint2(rx[j], ry[j]);
    }
}

template <int W>
hipError_t PathOps<W>::locate(TableView t, PackedView sv, UnitigBufs u, int k, uint64_t n_pos, uint64_t n_sym,
                              uint2* place, hipStream_t s) {
    static_assert(run_width(W) % 2 == 0, "two places per 16-byte store");
    if (!n_pos) return hipSuccess;
    if (n_sym < (uint64_t)k)  // PATH_NOWIN everywhere (its four bytes are equal)
        return hipMemsetAsync(place, (int)(PATH_NOWIN & 0xFF), n_pos * sizeof(uint2), s);
    const uint64_t threads = (n_pos + run_width(W) - 1) / run_width(W);
    hipLaunchKernelGGL(k_path_locate<W>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, t, sv, u, k, n_pos,
                       n_sym, place);
    return hipGetLastError();
}

}  // namespace kc
