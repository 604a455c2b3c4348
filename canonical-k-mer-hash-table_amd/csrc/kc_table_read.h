// kc_table_read.h -- reading a published full-key table, the counterpart of kc_table_insert.h:
// what every kernel that only reads the counted table shares (lookups, sequence queries, table
// algebra, read correction, compaction, the de Bruijn graph, the unitigs).
//
// The probe invariant.  table_insert (kc_table_insert.h) puts a key into the first free slot of its
// probe sequence -- the key's region, the buckets from its start bucket on, wrapping inside the
// region (kc_common.h) -- and no slot is ever freed.  So every bucket before the one that holds a
// key was full when the key went in and is full now: a probe that meets a bucket with a free slot
// without having met the key knows the table does not hold it.  A probe is therefore normally one
// 128-byte bucket read, present or absent, and never more than BPR.
//
// The readers are ordered after the counting passes, so every stored key is published: plain
// loads, no atomics on the table, no READY spinning (CNT_MASK takes the flag off the count word).
#pragma once
#include "kc_common.h"

namespace kc {

constexpr uint64_t NO_SLOT = ~0ULL;  // table_probe's miss where a hit is a slot index

DEV uint32_t tc_of(uint64_t cw, int count_mode) {  // T(c) of a count word: c mod 65536 (-m 0), else min(c, 16383)
    const uint64_t c = cw & CNT_MASK;
    return (uint32_t)(count_mode == 0 ? (c & 0xFFFF) : (c < 16383 ? c : 16383));
}

// a range on T(c): lo <= tc <= hi, hi 0 = no upper bound
DEV bool in_range(uint32_t tc, uint32_t lo, uint32_t hi) { return tc >= lo && (hi == 0 || tc <= hi); }

// one 128-byte bucket into registers: eight 16-byte loads issued together
DEV void load_bucket(const uint64_t* __restrict__ b, uint64_t (&bw)[BUCKET_WORDS]) {
    const uint4* b4 = reinterpret_cast<const uint4*>(b);
    uint4 v[BUCKET_WORDS / 2];
#pragma unroll
    for (int c = 0; c < BUCKET_WORDS / 2; c++) v[c] = b4[c];
#pragma unroll
    for (int c = 0; c < BUCKET_WORDS / 2; c++) {
        bw[2 * c] = ((uint64_t)v[c].y << 32) | v[c].x;
        bw[2 * c + 1] = ((uint64_t)v[c].w << 32) | v[c].z;
    }
}

// the key words of slot (bucket * S + slot in the bucket)
template <int W>
DEV void slot_tkey(const TableView& tv, uint64_t slot, uint64_t (&tk)[W]) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    const uint64_t bucket = slot / S;
    const uint64_t* key = tv.buckets + bucket * BUCKET_WORDS + (slot - bucket * S) * W;
#pragma unroll
    for (int i = 0; i < W; i++) tk[i] = key[i];
}

// the count word of that slot (CNT_MASK takes the READY flag off)
template <int W>
DEV uint64_t slot_count_word(const TableView& tv, uint64_t slot) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    const uint64_t bucket = slot / S;
    return tv.buckets[bucket * BUCKET_WORDS + S * W + (slot - bucket * S)];
}

// The probe of table key t, one thread per key: S strided loads of key word 0 per bucket, the other
// words only where word 0 matches.  hit(bucket, bk, sl) is called at the matching slot -- bucket its
// index, bk its words, sl the slot in it, whose count word is bk[S * W + sl] -- and its value
// returned; miss is returned at the first bucket with a free slot, or after BPR buckets.
// Its callers: table_count_word, graph_probe_slot (kc_graph_impl.h), cfind_built (kc_compact_impl.h).
// Three loops stay outside it, each with its reason: lookup_thread (kc_query_impl.h) and the two
// forms of 16 lanes per bucket, k_lookup_coop and lookup_coop (kc_seq_impl.h).
// The region's first bucket is formed once, outside the loop, and the bucket index only at the hit:
// with tv.buckets + (region * BPR + b) * BUCKET_WORDS in the loop k_neighbors<5, 7> lose an
// occupancy step (profiles/table_read_resources.md).
template <int W, class R, class F>
DEV R table_probe(const TableView& tv, const uint64_t (&t)[W], R miss, F&& hit) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    const uint64_t region = region_of(t[0], tv.R);
    const uint64_t* rb = tv.buckets + region * BPR * BUCKET_WORDS;  // the region's first bucket
    uint32_t b = bucket_in_region(t[0], tv.R);
    for (int probe = 0; probe < BPR; probe++) {
        const uint64_t* bk = rb + b * BUCKET_WORDS;
        bool free = false;
#pragma unroll
        for (int sl = 0; sl < S; sl++) {
            const uint64_t w0 = bk[sl * W];
            free |= w0 == EMPTY;
            if (w0 != t[0]) continue;
            bool eq = true;
#pragma unroll
            for (int i = 1; i < W; i++) eq &= bk[sl * W + i] == t[i];
            if (eq) return hit(region * BPR + b, bk, sl);
        }
        if (free) return miss;
        b = (b + 1) & (BPR - 1);
    }
    return miss;
}

// the count word of table key t in tv (found = false: the table does not hold it).  A one-word
// key's bucket is read whole, so the count word arrives with the keys: a measured choice of the
// table algebra, which the graph's neighbour probes share.
template <int W>
DEV uint64_t table_count_word(const TableView& tv, const uint64_t (&t)[W], bool& found) {
    constexpr int S = BUCKET_WORDS / (W + 1);
    found = false;
    if constexpr (W == 1) {
        const uint64_t region = region_of(t[0], tv.R);
        uint32_t b = bucket_in_region(t[0], tv.R);
        for (int probe = 0; probe < BPR; probe++) {
            uint64_t bw[BUCKET_WORDS];
            load_bucket(tv.buckets + (region * BPR + b) * BUCKET_WORDS, bw);
            bool free = false;
            uint64_t cw = 0;
#pragma unroll
            for (int sl = 0; sl < S; sl++) {
                free |= bw[sl] == EMPTY;
                if (bw[sl] == t[0]) {
                    found = true;
                    cw = bw[S + sl];
                }
            }
            if (found) return cw;
            if (free) return 0;
            b = (b + 1) & (BPR - 1);
        }
        return 0;
    } else {
        return table_probe<W>(tv, t, (uint64_t)0, [&](uint64_t, const uint64_t* bk, int sl) {
            found = true;
            return bk[S * W + sl];
        });
    }
}

}  // namespace kc
