// kc_slot_mask.h -- the 8-bit slot tags of level 3's LDS table (kc_count_impl.h k_p3) and the masks
// a probe takes from a bucket's tag word.  Plain C++ without a device call, host and device, so a
// stand-alone program checks it under the sanitizers against a byte-by-byte loop
// (tools/slot_mask_check.cpp).
//
// A bucket's tag word is one u64, byte s = the tag of slot s, 0 = empty.  A mask keeps the byte-lane
// form the exact zero-byte formula produces -- bit 7 of byte s set iff slot s is a candidate -- and
// is walked in place: SlotMask<S>::first(m) is the lowest candidate, rest(m) clears it.  (The masks
// were compacted to one bit per slot by a 32-bit multiply per half, twice per probe.)
#pragma once
#include <stdint.h>

#include <type_traits>

#if defined(__HIPCC__)
#define KC_SLOT_HD __host__ __device__ __forceinline__
#else
#define KC_SLOT_HD inline
#endif

namespace kc {

// the tag of a slot's key: 1..255 from the low byte of table key word 0 (0 = empty slot)
KC_SLOT_HD uint32_t slot_tag(uint64_t t0) { return 1u + (((uint32_t)t0 & 0xFFu) * 255u >> 8); }

// the tag in each of four bytes (both halves of a tag word compare against this one pattern)
KC_SLOT_HD uint32_t slot_tag4(uint32_t tag) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(0u, tag, 0u);  // byte 0 of tag into every byte
#else
    tag |= tag << 8;
    return tag | tag << 16;
#endif
}

// bit 7 of each zero byte of x (exact: no borrow between bytes)
KC_SLOT_HD uint32_t zero_byte_mask4(uint32_t x) {
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x | 0x7F7F7F7Fu);
}
KC_SLOT_HD uint64_t zero_byte_mask8(uint64_t x) {
    return zero_byte_mask4((uint32_t)x) | (uint64_t)zero_byte_mask4((uint32_t)(x >> 32)) << 32;
}

// The masks of a bucket of S slots.  S <= 4: only the low half of the tag word is live, and a mask
// is one 32-bit register.
template <int S>
struct SlotMask {
    static_assert(S >= 1 && S <= 8, "a tag word holds eight slots");
#ifdef KC_SLOT_MUTANT_SMASK
    static constexpr int LIVE = S < 8 ? S + 1 : S - 1;  // (the check's own mutation: one byte off)
#else
    static constexpr int LIVE = S;
#endif
    static constexpr bool HALF = S <= 4;
    typedef typename std::conditional<HALF, uint32_t, uint64_t>::type mask_t;
    // bit 7 of the first S bytes
    static constexpr uint64_t SMASK = 0x8080808080808080ULL >> (8 * (8 - LIVE));

    // slots whose tag is `tag` (t4 = slot_tag4(tag))
    static KC_SLOT_HD mask_t match(uint64_t tw, uint32_t t4) {
        if constexpr (HALF) return zero_byte_mask4((uint32_t)tw ^ t4) & (uint32_t)SMASK;
        else return zero_byte_mask8(tw ^ ((uint64_t)t4 << 32 | t4)) & SMASK;
    }
    // slots without a tag
    static KC_SLOT_HD mask_t empty(uint64_t tw) {
        if constexpr (HALF) return zero_byte_mask4((uint32_t)tw) & (uint32_t)SMASK;
        else return zero_byte_mask8(tw) & SMASK;
    }
    // 8 * (the lowest candidate slot): its byte offset among one-word keys, its tag's bit offset
    static KC_SLOT_HD uint32_t first8(mask_t m) {
        if constexpr (HALF) return (uint32_t)__builtin_ctz(m) & 0x38u;
        else return (uint32_t)__builtin_ctzll(m) & 0x38u;
    }
    static KC_SLOT_HD uint32_t first(mask_t m) { return first8(m) >> 3; }
    static KC_SLOT_HD mask_t rest(mask_t m) { return m & (m - 1); }
};

}  // namespace kc
