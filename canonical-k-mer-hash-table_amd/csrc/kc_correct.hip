// kc_correct.hip -- the width-independent kernels of the read correction (kc_correct*):
// k_correct_mark, per-position counts -> candidate positions, and k_correct_apply, verdicts -> the
// corrected text and the per-sequence counters; and the W-dispatch of k_correct_try
// (kc_correct_w.hip, one translation unit per key width).
#include "kc_correct_seq.h"

namespace kc {

// ---- k_correct_mark --------------------------------------------------------------------------------
// candidate(p): the window starts that cover p inside its sequence, [max(a, p - k + 1), min(p, b - k)],
// hold at least one valid window and no solid one.  A workgroup takes CORRECT_TILE positions and
// the CORRECT_HALO >= k - 1 before them, builds ONE inclusive prefix sum of (valid | solid << 16)
// over the CORRECT_TILE + CORRECT_HALO elements in LDS (both fields stay below 2^16) and answers
// every position with one subtraction.  (A position that is no base has no valid covering window,
// so the text itself is not read.)  Two threads find the tile's first and last sequence in the
// whole offset table, every position then searches only between those.
constexpr int MARK_E = CORRECT_TILE + CORRECT_HALO;
constexpr int MARK_PER = MARK_E / 256;
static_assert(MARK_E % 256 == 0 && CORRECT_HALO >= MAX_K - 1 && MARK_E < 65536, "mark tile geometry");

__global__ __launch_bounds__(256) void k_correct_mark(const uint32_t* __restrict__ cnt, uint64_t n_pos, uint64_t base,
                                                      const uint64_t* __restrict__ off, uint64_t i0, uint64_t i1, int k,
                                                      uint32_t smin, uint8_t* __restrict__ verdict) {
    __shared__ uint32_t ps[MARK_E];
    __shared__ uint32_t wsum[4];
    __shared__ uint64_t srange[2];
    const int tid = threadIdx.x;
    const uint64_t tile0 = (uint64_t)blockIdx.x * CORRECT_TILE;  // < n_pos
    // element e is position tile0 - CORRECT_HALO + e
    for (int e = tid; e < MARK_E; e += 256) {
        const uint64_t q = tile0 + (uint64_t)e;
        uint32_t x = 0;
        if (q >= (uint64_t)CORRECT_HALO && q - CORRECT_HALO < n_pos) {
            const uint32_t c = cnt[q - CORRECT_HALO];
            if (c != KC_NO_KMER) x = 1u + (c >= smin ? 0x10000u : 0u);
        }
        ps[e] = x;
    }
    if (tid == 0) srange[0] = correct_seq_of(off, i0, i1, base + tile0);
    if (tid == 64) {
        const uint64_t last = (tile0 + CORRECT_TILE < n_pos ? tile0 + CORRECT_TILE : n_pos) - 1;
        srange[1] = correct_seq_of(off, i0, i1, base + last) + 1;
    }
    __syncthreads();
    uint32_t v[MARK_PER], run = 0;
#pragma unroll
    for (int j = 0; j < MARK_PER; j++) v[j] = run += ps[tid * MARK_PER + j];
    const uint32_t incl = wave_incl_sum(run);
    if ((tid & 63) == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - run;
    for (int w = 0; w < (tid >> 6); w++) before += wsum[w];
#pragma unroll
    for (int j = 0; j < MARK_PER; j++) ps[tid * MARK_PER + j] = v[j] + before;
    __syncthreads();
    const uint64_t s0 = srange[0], s1 = srange[1];
#pragma unroll
    for (int j = 0; j < CORRECT_TILE / 256; j++) {
        const uint64_t p = tile0 + (uint64_t)(tid + 256 * j);
        if (p >= n_pos) continue;
        const uint64_t i = correct_seq_of(off, s0, s1, base + p);
        uint64_t lo, hi;
        bool cand = false;
        if (correct_cover(off[i] - base, off[i + 1] - base, p, k, lo, hi)) {
            // lo >= p - (k - 1) >= tile0 - CORRECT_HALO + 1: the element before lo exists
            const uint32_t d = ps[hi - tile0 + CORRECT_HALO] - ps[lo - tile0 + CORRECT_HALO - 1];
            cand = (d & 0xFFFFu) && !(d >> 16);
        }
        verdict[p] = cand ? CV_CAND : 0;
    }
}

hipError_t launch_correct_mark(const uint32_t* counts, uint64_t n_pos, uint64_t base, const uint64_t* off, uint64_t i0,
                               uint64_t i1, int k, uint32_t smin, uint8_t* verdict, hipStream_t s) {
    if (!n_pos) return hipSuccess;
    hipLaunchKernelGGL(k_correct_mark, dim3((unsigned)((n_pos + CORRECT_TILE - 1) / CORRECT_TILE)), dim3(256), 0, s,
                       counts, n_pos, base, off, i0, i1, k, smin, verdict);
    return hipGetLastError();
}

// ---- k_correct_apply -------------------------------------------------------------------------------
// One thread per position: an accepted position looks at the verdicts of the positions closer than
// k inside its sequence and is dropped when another accepted one is among them; out[p] is the
// accepted base in text[p]'s letter case, or text[p].  A thread reads and writes only its own byte
// of the text, so out == text works in place.  The four counters of a sequence are summed over the
// wave's lanes of that sequence (ballots) before one lane adds them: in an uncounted read every
// position is a candidate of the same sequence.
__global__ __launch_bounds__(256) void k_correct_apply(const uint8_t* text, uint8_t* out,
                                                       const uint8_t* __restrict__ verdict, uint64_t n_pos,
                                                       uint64_t base, const uint64_t* __restrict__ off, uint64_t i0,
                                                       uint64_t i1, int k, kc_correct_stat* __restrict__ stats) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    if (p - lane >= n_pos) return;  // the whole wave is past the end (wave-uniform)
    const bool in = p < n_pos;
    const uint8_t t = in ? text[p] : 0, v = in ? verdict[p] : 0;
    const bool cand = v & CV_CAND, acc = v & CV_ACC;
    uint64_t i = 0;
    bool dropped = false;
    if (cand) i = correct_seq_of(off, i0, i1, base + p);
    if (acc) {
        const uint64_t a = off[i] - base, b = off[i + 1] - base;
        const uint64_t lo = p + 1 >= a + (uint64_t)k ? p + 1 - (uint64_t)k : a;
        const uint64_t hi = p + (uint64_t)k <= b ? p + (uint64_t)k - 1 : b - 1;
        for (uint64_t q = lo; q <= hi && !dropped; q++) dropped = q != p && (verdict[q] & CV_ACC);
    }
    if (in) out[p] = acc && !dropped ? (uint8_t)("ACGT"[v & 3] | (t & 0x20)) : t;
    if (!stats) return;
    uint64_t pend = __ballot(cand);
    while (pend) {  // (wave-uniform)
        const int src = __ffsll((unsigned long long)pend) - 1;
        const uint64_t il = __shfl(i, src, 64);
        const bool mine = cand && i == il;
        const uint64_t m = __ballot(mine);
        const uint32_t n_cand = __popcll(m), n_fix = __popcll(__ballot(mine && acc && !dropped)),
                       n_amb = __popcll(__ballot(mine && (v & CV_AMBIG))), n_drop = __popcll(__ballot(mine && dropped));
        if (lane == src) {
            atomicAdd(&stats[il].candidates, n_cand);
            if (n_fix) atomicAdd(&stats[il].corrected, n_fix);
            if (n_amb) atomicAdd(&stats[il].ambiguous, n_amb);
            if (n_drop) atomicAdd(&stats[il].dropped, n_drop);
        }
        pend &= ~m;
    }
}

hipError_t launch_correct_apply(const uint8_t* text, uint8_t* out, const uint8_t* verdict, uint64_t n_pos,
                                uint64_t base, const uint64_t* off, uint64_t i0, uint64_t i1, int k,
                                kc_correct_stat* stats, hipStream_t s) {
    if (!n_pos) return hipSuccess;
    hipLaunchKernelGGL(k_correct_apply, dim3((unsigned)((n_pos + 255) / 256)), dim3(256), 0, s, text, out, verdict,
                       n_pos, base, off, i0, i1, k, stats);
    return hipGetLastError();
}

// W-dispatch of the try kernel (kc_correct_w.hip, one translation unit per key width)
hipError_t launch_correct_try(TableView t, PackedView sv, const uint32_t* counts, uint64_t n_pos, uint64_t base,
                              const uint64_t* off, uint64_t i0, uint64_t i1, int k, int count_mode, uint32_t smin,
                              uint8_t* verdict, hipStream_t s) {
    KC_DISPATCH(CorrectOps, t.W, attempt(t, sv, counts, n_pos, base, off, i0, i1, k, count_mode, smin, verdict, s));
}

}  // namespace kc
