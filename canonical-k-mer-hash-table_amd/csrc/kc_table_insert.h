// kc_table_insert.h -- the direct insert of one table key into the full-key table in HBM, shared
// by the counting kernels (kc_count_impl.h) and the table algebra (kc_join_impl.h).  The table's
// layout and the READY protocol of multi-word keys are described at the top of kc_count_impl.h;
// the readers' side of the probe invariant it keeps is kc_table_read.h.
#pragma once
#include "kc_common.h"

namespace kc {

// --------------------------------------------------------------------------------
// direct insert of one table key into the HBM table
// --------------------------------------------------------------------------------
template <int W>
DEV bool table_insert(const TableView& tv, const uint64_t (&tk)[W], uint64_t add = 1) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    const uint64_t region = region_of(tk[0], tv.R);
    uint32_t b = bucket_in_region(tk[0], tv.R);
    for (int probe = 0; probe < BPR; probe++) {
        uint64_t* bk = tv.buckets + (region * BPR + b) * BUCKET_WORDS;
        uint64_t w0[S];
        if constexpr (W == 1) {
            const uint4* b4 = reinterpret_cast<const uint4*>(bk);
#pragma unroll
            for (int q = 0; q < S / 2; q++) {
                uint4 v = b4[q];
                w0[2 * q] = ((uint64_t)v.y << 32) | v.x;
                w0[2 * q + 1] = ((uint64_t)v.w << 32) | v.z;
            }
        } else {
#pragma unroll
            for (int s = 0; s < S; s++) w0[s] = bk[s * W];
        }
        int s = 0;
        while (s < S) {
            uint64_t* kp = bk + s * W;
            uint64_t* cp = bk + S * W + s;
            uint64_t v0 = w0[s];
            if (v0 == EMPTY) {
                const uint64_t old = atomicCAS((unsigned long long*)kp, (unsigned long long)EMPTY,
                                               (unsigned long long)tk[0]);
                if (old == EMPTY) {
                    if constexpr (W == 1) {
                        atomicAdd((unsigned long long*)cp, (unsigned long long)add);
                    } else {
#pragma unroll
                        for (int i = 1; i < W; i++) atomic_store_agent(kp + i, tk[i]);
                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // words land before READY
                        atomicAdd((unsigned long long*)cp, (unsigned long long)(READY + add));
                    }
                    return true;
                }
                v0 = old;
                w0[s] = old;
            }
            if (v0 == tk[0]) {
                if constexpr (W == 1) {
                    atomicAdd((unsigned long long*)cp, (unsigned long long)add);
                    return true;
                } else {
                    const uint64_t c = atomic_load_agent(cp);
                    if (!(c & READY)) continue;  // claimed, not yet published: retry this slot
                    asm volatile("" ::: "memory");
                    bool eq = true;
#pragma unroll
                    for (int i = 1; i < W; i++) eq &= atomic_load_agent(kp + i) == tk[i];
                    if (eq) {
                        atomicAdd((unsigned long long*)cp, (unsigned long long)add);
                        return true;
                    }
                }
            }
            s++;
        }
        b = (b + 1) & (BPR - 1);
    }
    return false;  // region full
}

}  // namespace kc
