// kc_correct_seq.h -- what the read-correction kernels share (kc_correct.hip: mark, apply;
// kc_correct_impl.h: try): a position's sequence in the device offsets, and the window starts of
// that sequence that cover the position.
#pragma once
#include "kc_common.h"

namespace kc {

// The sequence that holds text byte pos: i in [lo, hi) with off[i] <= pos < off[i + 1] (empty
// sequences hold nothing).  The caller guarantees off[lo] <= pos < off[hi].
DEV uint64_t correct_seq_of(const uint64_t* __restrict__ off, uint64_t lo, uint64_t hi, uint64_t pos) {
    while (hi - lo > 1) {
        const uint64_t m = lo + (hi - lo) / 2;
        if (off[m] <= pos)
            lo = m;
        else
            hi = m;
    }
    return lo;
}

// the window starts that cover position p (pass-relative) inside the sequence [a, b): false if none
DEV bool correct_cover(uint64_t a, uint64_t b, uint64_t p, int k, uint64_t& lo, uint64_t& hi) {
    if (b - a < (uint64_t)k) return false;
    lo = p + 1 >= a + (uint64_t)k ? p + 1 - (uint64_t)k : a;  // max(a, p - k + 1)
    hi = p <= b - (uint64_t)k ? p : b - (uint64_t)k;          // min(p, b - k)
    return lo <= hi;
}

}  // namespace kc
