// kc_weak_rule.h -- the comparison of weak-link removal's rule (include/kc_api.h kc_cut_weak_device),
// as k_weak_verdict (kc_weak_impl.h) evaluates it.  Plain C++ without a device call, host and
// device, so a stand-alone program checks it under the sanitizers against 128-bit integers
// (tools/weak_rule_check.cpp): T(c) is below 2^16 in every count mode, so no graph a test can hold
// brings the products above 2^64.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define KC_WEAK_HD __host__ __device__ __forceinline__
#else
#define KC_WEAK_HD inline
#endif

namespace kc {

// the high word of x * y
KC_WEAK_HD uint64_t weak_mul_hi(uint64_t x, uint64_t y) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(x, y);
#else
    return (uint64_t)(((unsigned __int128)x * y) >> 64);
#endif
}

// local_n and local_sum of N(U): count_sum < 2^62 and eight entries at the most, so the sum is held
// as (hi, lo)
struct WeakLocal {
    uint64_t n, sum_lo, sum_hi;
};
KC_WEAK_HD void weak_local_add(WeakLocal& loc, uint64_t n, uint64_t sum) {
    loc.n += n;
    loc.sum_lo += sum;
    loc.sum_hi += loc.sum_lo < sum;
}

// count_sum(U) * local_n * 1000 < ratio_permille * local_sum * n(U), exactly: count_sum < 2^62, local_n
// < 2^33, local_sum < 2^65, n < 2^30 and ratio_permille <= 1000, so either side is below 2^106 and is
// held as (hi, lo)
KC_WEAK_HD bool weak_below(uint64_t count_sum, uint64_t n, const WeakLocal& loc, uint32_t ratio_permille) {
    const uint64_t h = weak_mul_hi(count_sum, loc.n), l = count_sum * loc.n;
    const uint64_t lh = weak_mul_hi(l, 1000) + h * 1000, ll = l * 1000;
    const uint64_t q = (uint64_t)ratio_permille * n;
    const uint64_t rh = weak_mul_hi(q, loc.sum_lo) + q * loc.sum_hi, rl = q * loc.sum_lo;
    return lh != rh ? lh < rh : ll < rl;
}

}  // namespace kc
