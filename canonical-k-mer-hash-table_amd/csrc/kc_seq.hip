// kc_seq.hip -- the width-independent kernels of the sequence queries (kc_text_counts*,
// kc_seq_stats*): k_seq_pack, text bytes -> a position-preserving packed stream, and k_seq_reduce,
// per-position counts -> per-sequence statistics; and the W-dispatch of k_seq_counts
// (kc_seq_w.hip, one translation unit per key width).
#include "kc_common.h"

namespace kc {

// ---- k_seq_pack ------------------------------------------------------------------------------------
// Symbol p of the stream is byte p of the text (nothing is removed, unlike the tokenizer, which
// drops FASTA newlines and headers): A/C/G/T in either case are bases, every other byte is a
// break.  The tokenizer's layout (PackedView): 32 symbols per pk word, big-endian, break bits at
// bit 31 - j of bk.  A thread packs 16 bytes, i.e. half a word; the even lane of a pair stores
// the word.  The nw = seq_pack_words(n) words are all written: the bytes past n -- the tail of
// the last text word and the padding word run_windows may read -- are breaks.
// The text may start at any byte address: a thread whose 16 bytes are not one aligned in-bounds
// 16-byte load reads the (at most five) aligned dwords that hold them and shifts.  An aligned
// dword that holds a byte of the text lies in that byte's page, so nothing is touched that the
// text's own pages do not hold.
__global__ __launch_bounds__(256) void k_seq_pack(const uint8_t* __restrict__ text, uint64_t n, uint64_t nw,
                                                  uint64_t* __restrict__ pk, uint32_t* __restrict__ bk) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t b0 = t * 16;
    uint32_t d[4] = {0, 0, 0, 0};  // the 16 bytes as little-endian dwords
    if (b0 < n) {
        const uintptr_t p = reinterpret_cast<uintptr_t>(text) + b0;
        if (!(p & 15) && b0 + 16 <= n) {
            const uint4 v = *reinterpret_cast<const uint4*>(p);
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        } else {
            const uintptr_t a = p & ~(uintptr_t)3, end = reinterpret_cast<uintptr_t>(text) + n;
            const int sh = (int)(p & 3) * 8;
            uint32_t r[5];
#pragma unroll
            for (int j = 0; j < 5; j++) r[j] = a + 4 * j < end ? *reinterpret_cast<const uint32_t*>(a + 4 * j) : 0;
#pragma unroll
            for (int j = 0; j < 4; j++) d[j] = sh ? (r[j] >> sh) | (r[j + 1] << (32 - sh)) : r[j];
        }
    }
    uint32_t sym = 0, brk = 0;  // 16 symbols at bits 30 - 2i, 16 break bits at bit 15 - i
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const uint8_t code = char_code((uint8_t)(d[i >> 2] >> (8 * (i & 3))));
        const bool bad = b0 + i >= n || code > 3;
        sym |= (bad ? 0u : (uint32_t)code) << (30 - 2 * i);
        brk |= (uint32_t)bad << (15 - i);
    }
    // (every lane reaches the shuffles: no thread has returned)
    const uint32_t sym_lo = __shfl_xor(sym, 1, 64), brk_lo = __shfl_xor(brk, 1, 64);
    const uint64_t w = t >> 1;
    if (!(t & 1) && w < nw) {
        pk[w] = ((uint64_t)sym << 32) | sym_lo;
        bk[w] = (brk << 16) | brk_lo;
    }
}

hipError_t launch_seq_pack(const uint8_t* text, uint64_t n, PackedView sv, hipStream_t s) {
    const uint64_t nw = seq_pack_words(n), threads = 2 * nw;
    hipLaunchKernelGGL(k_seq_pack, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, text, n, nw, sv.pk, sv.bk);
    return hipGetLastError();
}

// ---- k_seq_reduce ----------------------------------------------------------------------------------
// The statistics of one sequence from the per-position counts cnt[lo, hi) of its window starts
// (KC_NO_KMER: no window there): windows, present, solid, min, max and sum are wave reductions
// of one pass; the lower median, element (windows - 1) / 2 of the sorted values, is a two-pass
// radix select over the 16-bit values (T(c) < 65536): a 256-bin LDS histogram of the high bytes
// finds the median's high byte and its rank inside that bin, a second histogram of the low bytes
// of that bin's values finds the rest.  A team of NT threads works on one sequence: a wave (four
// sequences per 256-thread workgroup) for sequences of up to SEQ_WAVE_MAX bytes, the whole
// workgroup for longer ones.  All sums are integer, so the forms agree bit for bit.
// Every thread of the workgroup runs the same barriers, whatever its team's sequence.
struct SeqTeamLds {
    uint32_t hist[256];
    uint32_t sel[2];                // the selected bin, the rank inside it
    unsigned long long red[4][6];   // NT = 256: the four waves' partial reductions
};

// the bin of hist that holds rank r, and r's rank inside it, into L.sel (by the team's first wave)
DEV void seq_select(SeqTeamLds& L, uint32_t r, int tid) {
    if (tid < 64) {
        uint32_t h[4], s4 = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) s4 += h[b] = L.hist[4 * tid + b];
        const uint32_t incl = wave_incl_sum(s4);
        uint32_t acc = incl - s4;
        if (r >= acc && r < incl) {  // one lane
            bool done = false;
#pragma unroll
            for (int b = 0; b < 4; b++) {
                if (!done && r < acc + h[b]) {
                    L.sel[0] = 4 * tid + b;
                    L.sel[1] = r - acc;
                    done = true;
                }
                acc += h[b];
            }
        }
    }
    __syncthreads();
}

template <int NT>
DEV void seq_reduce_team(const uint32_t* __restrict__ cnt, uint64_t lo, uint64_t hi, uint32_t solid_min,
                         SeqTeamLds& L, int tid, kc_seq_stat* out) {
    for (int j = tid; j < 256; j += NT) L.hist[j] = 0;
    if (tid == 0) L.sel[0] = L.sel[1] = 0;
    __syncthreads();
    uint32_t windows = 0, present = 0, solid = 0, mn = 0xFFFFFFFFu, mx = 0;
    unsigned long long sum = 0;
    for (uint64_t p = lo + tid; p < hi; p += NT) {
        const uint32_t v = cnt[p];
        if (v == KC_NO_KMER) continue;
        windows++;
        present += v >= 1;
        solid += v >= solid_min;
        mn = min(mn, v);
        mx = max(mx, v);
        sum += v;
        atomicAdd(&L.hist[v >> 8], 1u);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        windows += __shfl_xor(windows, o, 64);
        present += __shfl_xor(present, o, 64);
        solid += __shfl_xor(solid, o, 64);
        mn = min(mn, (uint32_t)__shfl_xor(mn, o, 64));
        mx = max(mx, (uint32_t)__shfl_xor(mx, o, 64));
        sum += __shfl_xor(sum, o, 64);
    }
    if constexpr (NT == 256) {
        if ((tid & 63) == 0) {
            unsigned long long* r = L.red[tid >> 6];
            r[0] = windows; r[1] = present; r[2] = solid; r[3] = mn; r[4] = mx; r[5] = sum;
        }
    }
    __syncthreads();
    if constexpr (NT == 256) {
        windows = present = solid = mx = 0;
        mn = 0xFFFFFFFFu;
        sum = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const unsigned long long* r = L.red[w];
            windows += (uint32_t)r[0];
            present += (uint32_t)r[1];
            solid += (uint32_t)r[2];
            mn = min(mn, (uint32_t)r[3]);
            mx = max(mx, (uint32_t)r[4]);
            sum += r[5];
        }
    }
    // the high byte of the median
    seq_select(L, windows ? (windows - 1) / 2 : 0, tid);
    const uint32_t hb = L.sel[0], r2 = L.sel[1];
    __syncthreads();
    for (int j = tid; j < 256; j += NT) L.hist[j] = 0;
    __syncthreads();
    for (uint64_t p = lo + tid; p < hi; p += NT) {
        const uint32_t v = cnt[p];
        if ((v >> 8) == hb) atomicAdd(&L.hist[v & 255], 1u);  // (KC_NO_KMER has no such high part)
    }
    __syncthreads();
    seq_select(L, r2, tid);
    const uint32_t median = (hb << 8) | L.sel[0];
    if (tid == 0 && out) {
        kc_seq_stat st;
        st.windows = windows;
        st.present = present;
        st.solid = solid;
        st.min = windows ? mn : 0;
        st.median = windows ? median : 0;
        st.max = mx;
        st.sum = sum;
        *out = st;
    }
    __syncthreads();
}

// window starts of sequence [a, e) in a counts array that begins at text byte `base`
DEV void seq_window_range(uint64_t a, uint64_t e, uint64_t base, int k, uint64_t& lo, uint64_t& hi) {
    lo = hi = 0;
    if (e - a >= (uint64_t)k) {
        lo = a - base;
        hi = e - (uint64_t)k + 1 - base;  // p + k <= e
    }
}

// sequences i0 .. i1 - 1, one wave each; the longer ones are left to k_seq_reduce_long
__global__ __launch_bounds__(256) void k_seq_reduce(const uint32_t* __restrict__ cnt, uint64_t base,
                                                    const uint64_t* __restrict__ off, uint64_t i0, uint64_t i1, int k,
                                                    uint32_t solid_min, kc_seq_stat* __restrict__ stats) {
    __shared__ SeqTeamLds L[4];
    const int wave = threadIdx.x >> 6;
    const uint64_t i = i0 + (uint64_t)blockIdx.x * 4 + wave;
    uint64_t lo = 0, hi = 0;
    kc_seq_stat* out = nullptr;
    if (i < i1) {
        const uint64_t a = off[i], e = off[i + 1];
        if (e - a <= SEQ_WAVE_MAX) {
            out = stats + i;
            seq_window_range(a, e, base, k, lo, hi);
        }
    }
    seq_reduce_team<64>(cnt, lo, hi, solid_min, L[wave], threadIdx.x & 63, out);
}

__global__ __launch_bounds__(256) void k_seq_reduce_long(const uint32_t* __restrict__ cnt, uint64_t base,
                                                         const uint64_t* __restrict__ off,
                                                         const uint64_t* __restrict__ ids, int k, uint32_t solid_min,
                                                         kc_seq_stat* __restrict__ stats) {
    __shared__ SeqTeamLds L;
    const uint64_t i = ids[blockIdx.x];
    uint64_t lo, hi;
    seq_window_range(off[i], off[i + 1], base, k, lo, hi);
    seq_reduce_team<256>(cnt, lo, hi, solid_min, L, threadIdx.x, stats + i);
}

hipError_t launch_seq_reduce(const uint32_t* counts, uint64_t base, const uint64_t* off, uint64_t i0, uint64_t i1,
                             const uint64_t* long_ids, uint64_t n_long, int k, uint32_t solid_min, kc_seq_stat* stats,
                             hipStream_t s) {
    if (i1 > i0) {
        hipLaunchKernelGGL(k_seq_reduce, dim3((unsigned)((i1 - i0 + 3) / 4)), dim3(256), 0, s, counts, base, off, i0, i1,
                           k, solid_min, stats);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (n_long)
        hipLaunchKernelGGL(k_seq_reduce_long, dim3((unsigned)n_long), dim3(256), 0, s, counts, base, off, long_ids, k,
                           solid_min, stats);
    return hipGetLastError();
}

// W-dispatch of the per-position counts (kc_seq_w.hip, one translation unit per key width)
hipError_t launch_seq_counts(TableView t, PackedView sv, int k, int count_mode, uint64_t n_pos, uint64_t n_sym,
                             uint32_t* counts, hipStream_t s) {
    KC_DISPATCH(SeqOps, t.W, counts(t, sv, k, count_mode, n_pos, n_sym, counts, s));
}

}  // namespace kc
