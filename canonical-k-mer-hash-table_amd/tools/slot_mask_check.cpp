// slot_mask_check.cpp -- the slot tags and tag-word masks of level 3's insert (csrc/kc_slot_mask.h),
// the code k_p3 runs, in a program of its own against a byte-by-byte loop, for the sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -o bin/slot_mask_check tools/slot_mask_check.cpp
// (make bin/slot_mask_check; SLOTFLAGS=-DKC_SLOT_MUTANT_SMASK: the check's own mutation check, the
// constant of the first S bytes one byte off -- it must fail).  It touches no device and exits 0
// when every check holds.
//
// For every S in {1, 2, 3, 4, 5, 8}, every tag in 1..255 and every tag word whose eight bytes come
// from {0, tag, tag ^ 1, 0x80, 0xFF} (5^8 words per tag): the match mask and the empty mask, walked
// by first / rest, must give the slots the loop gives, in ascending order.
#include <cstdio>
#include <cstdlib>

#include "../csrc/kc_slot_mask.h"

using namespace kc;

// the reference: bit s set iff byte s of tw equals `byte`
static uint32_t loop_slots(uint64_t tw, uint32_t byte) {
    uint32_t r = 0;
    for (int s = 0; s < 8; s++)
        if (((tw >> (8 * s)) & 0xFF) == byte) r |= 1u << s;
    return r;
}

// the helpers' answer as the same bit set; false when the walk is not strictly ascending or leaves
// the tag word
template <int S>
static bool walk(typename SlotMask<S>::mask_t m, uint32_t& out) {
    typedef SlotMask<S> SM;
    out = 0;
    int last = -1;
    for (int n = 0; m; n++) {
        if (n == 8) return false;
        const uint32_t f8 = SM::first8(m), f = SM::first(m);
        if (f8 != 8 * f || f > 7 || (int)f <= last) return false;
        last = (int)f;
        out |= 1u << f;
        m = SM::rest(m);
    }
    return true;
}

static unsigned long long checked = 0, failed = 0, matches = 0, empties = 0;

// one tag word against a bucket of S slots: the loop's slots below S
template <int S>
static void one(uint64_t tw, uint32_t tag, uint32_t t4, uint32_t loop_m, uint32_t loop_e) {
    typedef SlotMask<S> SM;
    const uint32_t want_m = loop_m & ((1u << S) - 1), want_e = loop_e & ((1u << S) - 1);
    uint32_t got_m = 0, got_e = 0;
    const bool ok = walk<S>(SM::match(tw, t4), got_m) && walk<S>(SM::empty(tw), got_e) && got_m == want_m && got_e == want_e;
    checked++;
    matches += want_m != 0;
    empties += want_e != 0;
    if (!ok) {
        failed++;
        if (failed <= 5)
            std::printf("FAIL S %d tag %u word %016llx: match %02x want %02x, empty %02x want %02x\n", S, tag,
                        (unsigned long long)tw, got_m, want_m, got_e, want_e);
    }
}

static void sweep() {
    for (uint32_t tag = 1; tag <= 255; tag++) {
        const uint32_t t4 = slot_tag4(tag);
        if (t4 != tag * 0x01010101u) failed++;
        const uint8_t alphabet[5] = {0, (uint8_t)tag, (uint8_t)(tag ^ 1), 0x80, 0xFF};
        int digit[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        uint64_t tw = 0;  // every byte alphabet[0]
        for (;;) {
            const uint32_t loop_m = loop_slots(tw, tag), loop_e = loop_slots(tw, 0);
            one<1>(tw, tag, t4, loop_m, loop_e);
            one<2>(tw, tag, t4, loop_m, loop_e);
            one<3>(tw, tag, t4, loop_m, loop_e);
            one<4>(tw, tag, t4, loop_m, loop_e);
            one<5>(tw, tag, t4, loop_m, loop_e);
            one<8>(tw, tag, t4, loop_m, loop_e);
            int i = 0;  // the next word: an odometer over the alphabet
            for (; i < 8; i++) {
                digit[i] = digit[i] == 4 ? 0 : digit[i] + 1;
                tw = (tw & ~(0xFFULL << (8 * i))) | (uint64_t)alphabet[digit[i]] << (8 * i);
                if (digit[i]) break;
            }
            if (i == 8) break;
        }
    }
}

int main() {
    // the tag of a key: 1..255 from its low byte, every value taken
    bool seen[256] = {false};
    for (uint32_t b = 0; b < 256; b++) {
        const uint32_t t = slot_tag(0xABCDEF0123456700ULL | b);
        if (t < 1 || t > 255 || t != 1 + b * 255 / 256) failed++;
        seen[t] = true;
    }
    for (int t = 1; t <= 255; t++)
        if (!seen[t]) failed++;
    sweep();
    std::printf("slot_mask_check: %llu checked, %llu with a match, %llu with an empty slot, %llu failed\n", checked, matches,
                empties, failed);
    if (!matches || !empties || matches == checked || empties == checked) {
        std::printf("FAIL the sweep does not cover both answers\n");
        return 1;
    }
    return failed ? 1 : 0;
}
