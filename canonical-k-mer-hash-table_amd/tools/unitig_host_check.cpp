// unitig_host_check.cpp -- the host arithmetic of the unitig layer (csrc/kc_unitig_host.h) in a
// program of its own, for the sanitizers:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o bin/unitig_host_check tools/unitig_host_check.cpp
// (make bin/unitig_host_check).  It touches no device and exits 0 when every check holds.
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../csrc/kc_unitig_host.h"

#define CHECK(x)                                                          \
    do {                                                                  \
        if (!(x)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #x);  \
            return 1;                                                     \
        }                                                                 \
    } while (0)

int main() {
    using namespace kc;
    // rounds: ceil(log2(2 * bound)) + 1
    CHECK(unitig_rounds(0) == 2 && unitig_rounds(1) == 2 && unitig_rounds(2) == 3 && unitig_rounds(3) == 4);
    CHECK(unitig_rounds(19970) == 17);  // 2^15 < 39940 <= 2^16; the chain itself needs 15 of them
    CHECK(unitig_rounds(UNITIG_MAX_BOUND - 1) == 32 && unitig_rounds(UNITIG_MAX_BOUND) == 32);
    CHECK(unitig_rounds(~0ULL) == 64);  // (saturates instead of shifting past the word)
    for (uint64_t b = 1; b < 5000; b++) {
        const int r = unitig_rounds(b);
        CHECK((1ULL << (r - 1)) >= 2 * b && (r == 2 || (1ULL << (r - 2)) < 2 * b));
    }
    // scratch (two combinations no call asks for, beside the calls' own)
    const UnitigWants REC_VERDICT{true, true, false}, ANCHORS_ONLY{false, false, true};
    CHECK(unitig_scratch_bytes(0, 0) == 0 && unitig_scratch_bytes(1 << 20, 1000) == 5ULL * (1 << 20) + 140 * 1000);
    CHECK(unitig_scratch_bytes(268435456ULL, 86000000ULL) == 5 * 268435456ULL + 140 * 86000000ULL);
    CHECK(unitig_scratch_bytes(~0ULL, 1) == 0 && unitig_scratch_bytes(1, ~0ULL) == 0);
    CHECK(unitig_scratch_bytes(~0ULL / 5, ~0ULL / 140) == 0);
    // ... of kc_unitig_graph*: the record index per id on top
    CHECK(unitig_scratch_bytes(1 << 20, 1000, UNITIG_GRAPH) == 5ULL * (1 << 20) + 144 * 1000);
    CHECK(unitig_scratch_bytes(268435456ULL, 268435456ULL, UNITIG_GRAPH) == 149 * 268435456ULL);
    CHECK(unitig_scratch_bytes(1, ~0ULL / 144 + 1, UNITIG_GRAPH) == 0 && unitig_scratch_bytes(1, ~0ULL / 144 + 1) != 0);
    // ... of kc_clean*: the verdict byte per id on top
    CHECK(unitig_scratch_bytes(1 << 20, 1000, UNITIG_CLEAN) == 5ULL * (1 << 20) + 141 * 1000);
    CHECK(unitig_scratch_bytes(268435456ULL, 268435456ULL, UNITIG_CLEAN) == 146 * 268435456ULL);
    CHECK(unitig_scratch_bytes(1, ~0ULL / 141 + 1, UNITIG_CLEAN) == 0 && unitig_scratch_bytes(1, ~0ULL / 141 + 1) != 0);
    CHECK(unitig_scratch_bytes(1 << 20, 1000, REC_VERDICT) == 5ULL * (1 << 20) + 145 * 1000);
    // ... of kc_pop_bubbles*: the verdict byte and the two anchors per id on top
    CHECK(unitig_scratch_bytes(1 << 20, 1000, UNITIG_BUBBLE) == 5ULL * (1 << 20) + 149 * 1000);
    CHECK(unitig_scratch_bytes(268435456ULL, 268435456ULL, UNITIG_BUBBLE) == 154 * 268435456ULL);
    CHECK(unitig_scratch_bytes(1, ~0ULL / 149 + 1, UNITIG_BUBBLE) == 0 && unitig_scratch_bytes(1, ~0ULL / 149 + 1) != 0);
    CHECK(unitig_scratch_bytes(1 << 20, 1000, ANCHORS_ONLY) == 5ULL * (1 << 20) + 148 * 1000);
    // the layout: disjoint arrays, in order, inside `words`, and within the bytes the header states
    for (uint64_t b : std::vector<uint64_t>{1, 2, 3, 1000, 86000001, UNITIG_MAX_BOUND - 1}) {
        const UnitigLayout l = unitig_layout(b);
        const uint64_t half = (b + 1) / 2;
        CHECK(l.st0 == 0 && l.st1 - l.st0 == 6 * b && l.slot_of - l.st1 == 6 * b && l.off - l.slot_of == b);
        CHECK(l.succ - l.off == 2 * b && l.tc - l.succ == b && l.start - l.tc == half && l.pos - l.start == half);
        CHECK(l.words - l.pos == half && l.words * 8 <= UNITIG_NODE_BYTES * b + 24);
        CHECK(l.verdict == l.words);  // (no verdict bytes unless asked for)
        // with the verdict bytes: every earlier offset as it was, the bytes behind pos, inside the bytes stated
        const UnitigLayout v = unitig_layout(b, UNITIG_CLEAN);
        CHECK(v.st0 == l.st0 && v.st1 == l.st1 && v.slot_of == l.slot_of && v.off == l.off && v.succ == l.succ);
        CHECK(v.tc == l.tc && v.start == l.start && v.pos == l.pos && v.verdict == l.words);
        CHECK(v.words - v.verdict == (b + 7) / 8 && (v.words - v.verdict) * 8 >= b);
        CHECK(v.words * 8 <= (UNITIG_NODE_BYTES + UNITIG_VERDICT_BYTES) * b + 32);
        CHECK(l.anchors == l.words && v.anchors == v.words);  // (no anchors unless asked for)
        // with the anchors too: the verdict layout as it was, one word a node behind the verdict bytes
        const UnitigLayout a = unitig_layout(b, UNITIG_BUBBLE);
        CHECK(a.st0 == v.st0 && a.st1 == v.st1 && a.slot_of == v.slot_of && a.off == v.off && a.succ == v.succ);
        CHECK(a.tc == v.tc && a.start == v.start && a.pos == v.pos && a.verdict == v.verdict && a.anchors == v.words);
        CHECK(a.words - a.anchors == b && (a.words - a.anchors) * 8 == UNITIG_ANCHOR_BYTES * b);
        CHECK(a.words * 8 <= (UNITIG_NODE_BYTES + UNITIG_VERDICT_BYTES + UNITIG_ANCHOR_BYTES) * b + 32);
    }
    // every combination: the bytes per id add up, and only the verdict bytes and the anchors add words
    for (int m = 0; m < 8; m++)
        for (uint64_t b : std::vector<uint64_t>{1, 7, 1000}) {
            const UnitigWants w{(m & 1) != 0, (m & 2) != 0, (m & 4) != 0};
            const uint64_t slots = 1 << 14;
            CHECK(unitig_scratch_bytes(slots, b, w) == 5 * slots + (140 + 4 * w.rec + 1 * w.verdict + 8 * w.anchors) * b);
            CHECK(unitig_layout(b, w).words == unitig_layout(b).words + (w.verdict ? (b + 7) / 8 : 0) + (w.anchors ? b : 0));
        }
    {  // every word of a small layout belongs to exactly one array
        const uint64_t b = 7;
        const UnitigLayout l = unitig_layout(b);
        std::vector<int> owner(l.words, 0);
        const uint64_t at[] = {l.st0, l.st1, l.slot_of, l.off, l.succ, l.tc, l.start, l.pos};
        const uint64_t len[] = {6 * b, 6 * b, b, 2 * b, b, 4, 4, 4};
        for (int a = 0; a < 8; a++)
            for (uint64_t w = 0; w < len[a]; w++) owner[at[a] + w]++;
        for (int o : owner) CHECK(o == 1);
        // ... and of the layout with verdict bytes: one more word for seven of them
        const UnitigLayout v = unitig_layout(b, UNITIG_CLEAN);
        std::vector<int> owner_v(v.words, 0);
        for (int a = 0; a < 8; a++)
            for (uint64_t w = 0; w < len[a]; w++) owner_v[at[a] + w]++;
        for (uint64_t w = 0; w < (b + 7) / 8; w++) owner_v[v.verdict + w]++;
        for (int o : owner_v) CHECK(o == 1);
        // ... and with the anchors: b more words
        const UnitigLayout a = unitig_layout(b, UNITIG_BUBBLE);
        std::vector<int> owner_a(a.words, 0);
        for (int x = 0; x < 8; x++)
            for (uint64_t w = 0; w < len[x]; w++) owner_a[at[x] + w]++;
        for (uint64_t w = 0; w < (b + 7) / 8; w++) owner_a[a.verdict + w]++;
        for (uint64_t w = 0; w < b; w++) owner_a[a.anchors + w]++;
        for (int o : owner_a) CHECK(o == 1);
    }
    // the FASTA header
    char buf[160];
    int n = unitig_fasta_header(buf, sizeof buf, 0, 3, 10, 31, false);
    CHECK(n == (int)std::strlen(buf) && std::string(buf) == ">0 LN:i:33 KC:i:10 km:f:3.3");
    unitig_fasta_header(buf, sizeof buf, 17, 2, 50, 31, true);
    CHECK(std::string(buf) == ">17 LN:i:32 KC:i:50 km:f:25.0 circular");
    n = unitig_fasta_header(buf, sizeof buf, ~0ULL, ~0ULL - 600, ~0ULL, 479, true);  // the longest it gets
    CHECK(n > 0 && n < (int)sizeof buf && n == (int)std::strlen(buf));
    char tiny[8];
    n = unitig_fasta_header(tiny, sizeof tiny, 123456, 5, 5, 31, false);  // truncated, never past the buffer
    CHECK(n > (int)sizeof tiny && std::strlen(tiny) == sizeof tiny - 1);
    unitig_fasta_header(buf, sizeof buf, 1, 0, 0, 0, false);  // no division by zero
    CHECK(std::string(buf) == ">1 LN:i:0 KC:i:0 km:f:0.0");
    std::puts("unitig_host_check: OK");
    return 0;
}
