/*
 * kc_api.h -- C ABI of the MI355X canonical k-mer counting engine
 * (canonical-k-mer-hash-table_amd/lib/libkc.so).
 *
 * This is the drop-in boundary for the hot path of Kaarme
 * (Denopia/canonical-k-mer-hash-table): parallel_parser -> kmer_factory ->
 * kmer_hash_table (+ double_bloomfilter).  The reference has no FFI; its internal
 * seams are the per-chunk worker call hash_kmers(chunk, format)
 * (include/parallel_parser.hpp:1302-1479), the per-k-mer table call
 * process_kmer_MT (include/kmer_hash_table.hpp:308, source/kmer_hash_table.cpp:2207)
 * and the writers (source/kmer_hash_table.cpp:2013-2050, 4318-4524).  Each entry
 * point below names the reference interface it replaces.
 *
 * Conventions: plain pointers and sizes, no C++ or torch types.  Every call
 * returns 0 (KC_OK) or a negative KC_ERR_*; the library never exit()s (the
 * reference does, e.g. kmer_hash_table.cpp:2552-2556) -- kc_last_error() gives
 * the message.  A context owns all device memory and is used by one host thread
 * at a time.  Host buffers passed to *_chunk calls are copied before return.
 */
#ifndef KC_API_H
#define KC_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Largest k-mer length: keys of up to fifteen 64-bit words, which with their count fill
   one 128-byte table bucket (the reference sizes its blocks dynamically,
   kmer_factory.cpp:33, and accepts any k > 0, main.cpp:135; INTEGRATION.md "Differences"
   states this bound). */
#define KC_MAX_K 479

#define KC_OK 0
#define KC_ERR_ARG (-1)         /* invalid argument */
#define KC_ERR_HIP (-2)         /* HIP runtime / device error */
#define KC_ERR_TABLE_FULL (-3)  /* "Hash table is full" (kmer_hash_table.cpp:2552-2556) */
#define KC_ERR_STATE (-4)       /* call out of order (e.g. count before bloom finalize) */
#define KC_ERR_IO (-5)          /* file error */
#define KC_ERR_NOMEM (-6)       /* host or device allocation failed */
#define KC_ERR_UNSUPPORTED (-7) /* the Bloom filter on the per-window routing entry point kc_route_device (a sharded
                                   Bloom job routes {key, count} records to the filter's owner instead:
                                   kc_bloom_records_device); the compact representation of a -m 0 table */

/* input_mode of main.cpp:178-189 */
#define KC_FMT_FASTA 0
#define KC_FMT_FASTQ 1
#define KC_FMT_PLAIN 2

typedef struct kc_ctx kc_ctx;

/* Replaces the CLI-derived arguments struct (main.cpp:70-99) that main() hands to
 * the parse_input_* functors (main.cpp:468-543). */
typedef struct {
    int32_t k;              /* KLEN, 1..KC_MAX_K (the reference is wrong for k % 32 == 0) */
    int32_t mode;           /* -m: 0 plain table (uint16 counts wrap), 1/2 kaarme (saturate at 16383) */
    int32_t bf_enable;      /* -b: two-pass double Bloom filter prefilter */
    int32_t device;         /* HIP device ordinal */
    uint64_t table_slots;   /* -s: minimum hash table slots (ignored with bf_enable: 2 * new_in_second) */
    uint64_t est_unique;    /* -u: estimated unique k-mers, sizes the Bloom filter */
    double fpr;             /* -f: Bloom filter false positive rate (0.001..0.999) */
    uint64_t min_abundance; /* -a: output threshold on T(c) */
    uint64_t batch_bytes;   /* staging batch size in bytes (0 = 256 MiB) */
} kc_config;

/* One reference chunk (text_chunk, include/text_reader.h:17-36): `len` bytes at
 * `off` of a file image, processed with `broken_header`. */
typedef struct {
    uint64_t off;
    uint64_t len;
    int32_t broken_header;
    int32_t pad;
} kc_chunk;

typedef struct {
    uint64_t windows;         /* k-mer windows of the counting pass */
    uint64_t inserted;        /* windows inserted (all windows without BF; gate-passing with BF) */
    uint64_t distinct;        /* occupied table slots ("Main array slots used", parallel_parser.hpp:1551-1562) */
    uint64_t table_slots;     /* slot capacity of the device table */
    uint64_t bf_windows;      /* k-mer windows of Bloom pass 1 */
    uint64_t bf_bits;         /* bits per Bloom filter (main.cpp:402-418) */
    uint64_t new_in_first;    /* DoubleAtomicDoubleBloomFilter counters (double_bloomfilter.hpp:233-246) */
    uint64_t new_in_second;
    uint64_t failed_in_first;
    uint64_t chunks;          /* chunks processed by the counting pass */
    uint64_t bytes;           /* input bytes processed by the counting pass */
    uint64_t part_fallbacks;  /* partitioned batches redone on the exact layout (a full skew list) */
    uint64_t spilled;         /* keys past their segment's end, inserted through the exact levels */
    uint64_t heavy_records;   /* {k-mer, count} records of repeated windows (homopolymer runs) */
    uint64_t reused_passes;   /* counting passes that started from the Bloom pass's kept partitions */
    uint64_t reuse_level;     /* the partition level the last reused pass started from: 2 (level 3 only),
                                 1 (levels 2-3), 0 = no reuse */
    uint64_t route_counts_kept; /* kc_route_table_device calls that took the per-block owner counts the
                                   counting passes kept (kc_route_hint) instead of running a count pass */
    uint64_t deferred_level3;   /* level-3 passes of counting passes over several staging batches that
                                   inserted a group of batches' level-2 partitions at once (one table
                                   sweep per group, not per batch; KC_DEFER=0 disables it) */
} kc_stats;

/* Creates the device table (PointerHashTableCanonicalAV ctor,
 * kmer_hash_table.cpp:2128-2150 / BasicAtomicFlagHashTableLong, 1992-2003) and,
 * with bf_enable, the Bloom filter (DoubleAtomicDoubleBloomFilter ctor,
 * double_bloomfilter.hpp:255-260 sized as main.cpp:402-431). */
int kc_create(const kc_config* cfg, kc_ctx** out);
void kc_destroy(kc_ctx* ctx);
/* Message of the last failed call on ctx (or of kc_create when ctx == NULL). */
const char* kc_last_error(const kc_ctx* ctx);

/* Bloom pass 1 over one chunk: bloom_filter_kmers(chunk, format)
 * (parallel_parser.hpp:2788-2940) -> insertion_process per k-mer. */
int kc_bloom_chunk(kc_ctx* ctx, const uint8_t* buf, size_t len, int fmt, int broken_header);
/* End of pass 1: main.cpp:454-461 (min_slots = 2 * new_in_second; resize()).
 * Sizes and allocates the table. */
int kc_bloom_finalize(kc_ctx* ctx, uint64_t* new_in_second);
/* Counting pass over one chunk: hash_kmers(chunk, format) (parallel_parser.hpp:1302-1479)
 * calling process_kmer_MT per window (kmer_hash_table.cpp:2207) -- behind the Bloom
 * gate (parallel_parser.hpp:2436-2453) when bf_enable and mode != 1. */
int kc_count_chunk(kc_ctx* ctx, const uint8_t* buf, size_t len, int fmt, int broken_header);

/* The same two passes over a DEVICE-resident file image and a chunk table
 * (kc_plan_chunks), enqueued on hip_stream (a hipStream_t; NULL = the HIP null
 * stream) after the work already queued there, so a buffer produced on that stream
 * (e.g. by PyTorch on its current stream) is safe to pass.  The image must stay valid
 * until the work completes (kc_sync).  Every *_device entry point follows this rule.
 * Host waits inside these two calls (the work is still ordered on hip_stream):
 *   - an image that fits one staging batch (kc_config.batch_bytes): the call returns once
 *     the batch's single-pass levels have run -- it reads two device counters (skew list,
 *     segment overflow) to launch the batch's fallback work only when it is needed;
 *   - an image of several batches: before batch i+1 is queued, the call waits until batch i's
 *     chunk descriptors have reached the device (queued after the work before it), so at most
 *     one batch is queued ahead; the fallback work stays behind a device-side gate.  A counting
 *     pass of several batches defers level 3 (kc_stats.deferred_level3): the level-2 partitions
 *     of a group of batches wait in HBM and one level-3 pass inserts them (one sweep of the
 *     table per group, not per batch; KC_DEFER=0 disables it); the call then waits for each
 *     batch's partition levels (it reads the batch's skew-list and overflow counters);
 *   - the counting pass that reuses the Bloom pass's partitions waits for its work (below).
 * Level-1 reuse: when the Bloom pass is one staging batch, it keeps its window
 * partition, and a counting pass given the same image pointer, chunk table and format
 * -- and the same bytes, checked by a checksum of the chunks -- starts from that
 * partition instead of tokenizing and canonicalising every window again (that counting
 * call then waits for its work; kc_stats.reused_passes counts such passes).  Any
 * difference runs the ordinary counting pass.  KC_REUSE=0 disables it. */
int kc_bloom_device(kc_ctx* ctx, const uint8_t* dev_image, const kc_chunk* chunks, size_t n_chunks, int fmt,
                    void* hip_stream);
int kc_count_device(kc_ctx* ctx, const uint8_t* dev_image, const kc_chunk* chunks, size_t n_chunks, int fmt,
                    void* hip_stream);
/* Distinct-count estimate of a device image (no reference counterpart: Kaarme takes the
 * table size from its user, -s, main.cpp:134-154, or from the Bloom pass, main.cpp:454): the
 * canonical k-mers of the image's windows into a HyperLogLog sketch of 2^14 registers
 * (~0.8 % standard error; for k <= 128 over a 1/8 sample of the distinct k-mers picked by a
 * strand-symmetric hash, the estimate scaled by 8, whose sampling error is far smaller for
 * the millions of k-mers it is meant for and ~9 % at a thousand), so a caller can size a
 * table (kc_config.table_slots) before
 * counting, e.g. a rank's local table in a sharded job.  Counts nothing and leaves the
 * table alone; the call waits for its work (the estimate is a host value).  Any context of
 * the same k can run it (its table size does not matter).  When HBM allows, the context keeps
 * the tokenized batches (3/8 byte per input byte) for its next kc_count_device over the same
 * image pointer, chunk table and format, which then skips its tokenizer: the caller must not
 * change the image's bytes in between (kc_reset or any other pass drops them). */
int kc_estimate_distinct_device(kc_ctx* ctx, const uint8_t* dev_image, const kc_chunk* chunks, size_t n_chunks,
                                int fmt, void* hip_stream, double* estimate);
/* Size the device table of the job about to be counted (after kc_create or kc_reset, before
 * its first counting pass; no Bloom filter): `slots` k-mers with the usual 25 % headroom,
 * e.g. 1.1 x kc_estimate_distinct_device, instead of -s (kc_config.table_slots), which stays
 * the job's reference capacity (KC_STRICT_CAPACITY: kc_finish fails past next_prime3mod4(-s)).
 * 0 = back to -s.
 * A table much smaller than its allocation gets a new one (the memory goes back to the
 * deferred level 3).  Replaces nothing in the reference, whose table is -s slots
 * (parallel_parser.hpp:1192-1196): -s 2.6e9 for C4's 1.0 G distinct k-mers takes 83 GB of
 * HBM at 25 % headroom, the estimate 35 GB. */
int kc_size_table(kc_ctx* ctx, uint64_t slots);
/* Wait for all work enqueued on the context. */
int kc_sync(kc_ctx* ctx);

/* Multi-GPU hash-prefix sharding (the reference is single-process):
 * kc_route_device tokenizes a device image (its chunks must fit one staging batch) and
 * writes the table keys of its windows to dev_out grouped by owner shard (kc_key_words()
 * u64 per key, the engine's internal bijective key encoding); counts[d] = keys for
 * shard d.  out_capacity (keys) must be >= the image bytes + chunks.  The caller
 * exchanges the groups (all-to-all) and every owner inserts what it received with
 * kc_insert_keys_device.  Not available with the Bloom filter. */
int kc_route_device(kc_ctx* ctx, const uint8_t* dev_image, const kc_chunk* chunks, size_t n_chunks, int fmt,
                    uint32_t nshards, uint64_t* dev_out, uint64_t out_capacity, uint64_t* counts, void* hip_stream);
int kc_insert_keys_device(kc_ctx* ctx, const uint64_t* dev_keys, uint64_t n_keys, void* hip_stream);

/* Super-k-mer sharding (the multi-GPU exchange of kaarme_amd.sharded): the owner of
 * a canonical k-mer is a hash of its canonical minimizer (the least h(canonical m-mer) over its
 * k - m + 1 m-mers; m = 0: min(15, k)), the same for both strands, so every occurrence of a k-mer
 * has one owner and the owners' counts are exact.  kc_route_superkmers_device tokenizes a device
 * image (any number of staging batches) and writes, per owner o < nshards (<= 64), the maximal runs
 * of consecutive windows with owner o ("super-k-mers": a break symbol + the run's k - 1 + r symbols)
 * as a packed symbol stream -- pk words of 32 2-bit symbols, bk words of their break flags (bit 31 =
 * the word's first symbol), the tokenizer's layout -- into region o of dev_pk / dev_bk (cap_words
 * words per region, region o at o * cap_words); words[o] = words written (or needed), windows[o] =
 * windows routed.  cap_words = 0: a dry run that only sizes the regions; a region too small fails
 * with KC_ERR_NOMEM and words[] holding the sizes needed.  The caller exchanges region o with
 * rank o (all-to-all), and each owner counts what it received with kc_count_packed_device (or runs
 * its Bloom pass 1 over it with kc_bloom_packed_device, then kc_bloom_finalize and the counting
 * pass): the concatenated streams of every sender, n_words words, readable for n_words + 2 words;
 * `windows` = the windows they hold, a hint (0 = unknown) that only chooses the length of the batches
 * the stream is cut into (about a staging batch's windows each if the stream is uniform).  It sizes
 * no buffer: every batch's windows are counted on the device before its partition levels are sized
 * (one read of the break words and one host wait per call), so any value gives the same table, and
 * a stream whose windows cluster (mixed read lengths, runs of N) is as safe as a uniform one.  A hint
 * far below the truth makes long batches, which may end in KC_ERR_NOMEM.
 * kc_packed_windows_device is that counter on its own: *windows = the windows of dev_bk[0 .. n_words),
 * i.e. the sum of max(0, L - k + 1) over its maximal break-free runs of L symbols (the word before
 * the range counts as a break; dev_pk is not read); it waits for the stream.  Replaces the
 * reference's one shared table (kmer_hash_table.cpp:2207-2567) with one table per owner. */
int kc_route_superkmers_device(kc_ctx* ctx, const uint8_t* dev_image, const kc_chunk* chunks, size_t n_chunks,
                               int fmt, uint32_t nshards, int m, uint64_t* dev_pk, uint32_t* dev_bk,
                               uint64_t cap_words, uint64_t* words, uint64_t* windows, void* hip_stream);
int kc_count_packed_device(kc_ctx* ctx, const uint64_t* dev_pk, const uint32_t* dev_bk, uint64_t n_words,
                           uint64_t windows, void* hip_stream);
int kc_bloom_packed_device(kc_ctx* ctx, const uint64_t* dev_pk, const uint32_t* dev_bk, uint64_t n_words,
                           uint64_t windows, void* hip_stream);
int kc_packed_windows_device(kc_ctx* ctx, const uint64_t* dev_pk, const uint32_t* dev_bk, uint64_t n_words,
                             void* hip_stream, uint64_t* windows);

/* Pre-aggregated sharding (the multi-GPU path of kaarme_amd.sharded): every rank counts
 * its own input into its own table, then kc_route_table_device writes the table's
 * occupied slots as records {W table-key words, raw count} grouped by owner shard
 * (the owner_of bit field of word 0) into dev_out (capacity in records; NULL = counts
 * only) and the per-owner record counts into counts[nshards] (nshards <= 64); after
 * the exchange kc_insert_counts_device adds received records into the owner's table.
 * Replaces the reference's single shared table (kmer_hash_table.cpp:2207-2567): the union
 * of the owners' tables is the count of the whole input. */
int kc_route_table_device(kc_ctx* ctx, uint32_t nshards, uint64_t* dev_out, uint64_t out_capacity,
                          uint64_t* counts, void* hip_stream);
/* Tells the context that its table will be routed to nshards (1..64) owners (0 = off): every
 * level-3 pass of the counting pipeline then also writes its region's record counts per owner
 * (the two 256-bucket blocks the route reads), so a kc_route_table_device(nshards) after
 * counting passes that all went through level 3 (the partitioned path; not the direct
 * small-batch path or the merge inserts) runs no count pass over the table -- one streaming
 * read of the table fewer per merge.  kc_stats.route_counts_kept counts
 * such routes.  The records and counts are the same either way. */
int kc_route_hint(kc_ctx* ctx, uint32_t nshards);
int kc_insert_counts_device(kc_ctx* ctx, const uint64_t* dev_records, uint64_t n_records, void* hip_stream);
/* The same for records that arrive as ngroups (<= 64) consecutive groups of
 * group_counts[g] records (host array), one per sending rank, each in the order
 * kc_route_table_device wrote it: sorted by region when the sender's table has this
 * table's size.  The table is then updated in one LDS pass per region over the groups'
 * region runs (no partition levels); groups that are not sorted take
 * kc_insert_counts_device. */
int kc_insert_counts_runs_device(kc_ctx* ctx, const uint64_t* dev_records, const uint64_t* group_counts,
                                 uint32_t ngroups, void* hip_stream);

/* Whole-filter primitives (the reference has one filter,
 * DoubleAtomicDoubleBloomFilter, double_bloomfilter.hpp:233-260, filled by every worker of
 * the Bloom pass, parallel_parser.hpp:2788-2940), for a caller that runs kc_bloom_device on
 * every rank and combines the ranks' whole filters itself.  (kaarme_amd.sharded does not: it
 * shards the filter by the k-mers' owner, kc_bloom_records_device / kc_count_records_device
 * below, so no filter crosses xGMI.)  The primitives:
 *   kc_bloom_get_device   copies words [first_word, first_word + n_words) of the filter to
 *                         dev_dst (after the work queued on hip_stream and the context);
 *   kc_bloom_merge_device combines nparts copies of one word range (consecutive in
 *                         dev_parts, n_words each; whole 16-word blocks in the blocked
 *                         layout) into dev_out: filter 1 = OR, filter 2 = OR | (filter-1
 *                         bits set in >= 2 copies), so every k-mer seen twice in the whole
 *                         input passes the gate (seen twice on one rank, or on two ranks);
 *   kc_bloom_set_device   replaces the whole filter (n_words = kc_bloom_info's count) and
 *                         sets the pass-1 counter new_in_second, which kc_bloom_finalize
 *                         sizes the table from (main.cpp:454), to kc_bloom_estimate of the
 *                         new filter (also returned in *new_in_second; the same on every rank
 *                         for the combined filter); new_in_first / failed_in_first stay the
 *                         rank's own;
 *   kc_bloom_estimate     the number of distinct k-mers in filter 2 estimated from its set
 *                         bits (X of m bits, h pass-1 positions: -(m/h) ln(1 - X/m)). */
int kc_bloom_get_device(kc_ctx* ctx, uint32_t* dev_dst, uint64_t first_word, uint64_t n_words, void* hip_stream);
int kc_bloom_merge_device(kc_ctx* ctx, const uint32_t* dev_parts, uint32_t nparts, uint64_t n_words,
                          uint32_t* dev_out, void* hip_stream);
int kc_bloom_set_device(kc_ctx* ctx, const uint32_t* dev_src, uint64_t n_words, uint64_t* new_in_second,
                        void* hip_stream);
int kc_bloom_estimate(kc_ctx* ctx, uint64_t* distinct_in_second, void* hip_stream);

/* Owner-sharded Bloom filter ("the BF is sharded by the same owner"): the two
 * passes of a Bloom job over pre-aggregated records {W table-key words, raw count} -- what
 * kc_route_table_device writes from an ungated local count and the exchange delivers to the
 * k-mers' owner -- on the owner's context (its filter sized for its 1/G share of -u):
 *   kc_bloom_records_device   Bloom pass 1 (before kc_bloom_finalize) over records of
 *                             DISTINCT keys (the senders' records of one k-mer summed first:
 *                             kaarme_amd.sharded aggregates them in a table): insertion_process
 *                             (double_bloomfilter.hpp:371-413) twice for a record of count >= 2
 *                             -- a k-mer seen at least twice sets its filter-2 bits -- then once
 *                             for every record of count 1, as in one sequential order of the
 *                             reference's pass (parallel_parser.hpp:2788-2940), so a singleton
 *                             meets one filter;
 *   kc_count_records_device   the counting pass (after kc_bloom_finalize, which sizes the table
 *                             2 * new_in_second, main.cpp:454): adds each record's count when
 *                             its filter-2 bits pass the gate (parallel_parser.hpp:2436-2453);
 *                             -m 1 -b and contexts without the filter add every record.
 * Blocked filter layout only (the reference layout hashes the Rabin-Karp root, which a table
 * key does not carry): KC_ERR_ARG otherwise. */
int kc_bloom_records_device(kc_ctx* ctx, const uint64_t* dev_records, uint64_t n_records, void* hip_stream);
int kc_count_records_device(kc_ctx* ctx, const uint64_t* dev_records, uint64_t n_records, void* hip_stream);

/* Kaarme's compact representation: PointerHashTableCanonicalAV's 8-byte
 * slot words (OneCharacterAndPointerKMerAtomicVariable, kmer.hpp:103-149: occupied, predecessor
 * exists, self / predecessor canonical during insertion, left and right character, 14-bit count,
 * 38-bit predecessor slot) plus a secondary array of the chain starts' full keys, built from the
 * counted table after the counting pass (the reference builds it while inserting,
 * kmer_hash_table.cpp:2207-2567).  Every k-mer links to a k-mer of the table that precedes it on
 * the strand its minimizer reads forward, so the reference's walk (reconstruct_kmer_in_slot,
 * kmer_hash_table.cpp:3848-4058) rebuilds it in at most k - 2 hops.  -m 1 / -m 2 only (14-bit
 * counts); a snapshot: later counting does not update it, kc_reset drops it.
 *   kc_compact        builds it at the given load (slots = k-mers / load; 0 = 0.8);
 *   kc_compact_dump   reconstructs every k-mer with T(c) >= a: records as kc_dump, plus the
 *                     longest and the mean walk (hops);
 *   kc_compact_lookup T(c) of canonical keys (host arrays, kc_key_words() words each, the
 *                     kc_dump key layout) from the compact words alone, 0 if absent;
 *   kc_compact_read   copies the slot words and the secondary array's words to the host. */
typedef struct {
    uint64_t slots;         /* slot words (8 bytes each) */
    uint64_t kmers;         /* k-mers held (the table's distinct k-mers) */
    uint64_t chain_starts;  /* k-mers without a predecessor: full keys in the secondary array */
    uint64_t bytes;         /* slot words + secondary array */
    uint64_t table_bytes;   /* the full-key table it was built from */
} kc_compact_info;
int kc_compact(kc_ctx* ctx, double load, kc_compact_info* info);
int kc_compact_dump(kc_ctx* ctx, uint64_t** records, uint64_t* n_records, uint64_t* max_hops, double* mean_hops);
int kc_compact_lookup(kc_ctx* ctx, const uint64_t* keys, uint64_t n, uint32_t* counts);
int kc_compact_read(kc_ctx* ctx, uint64_t* words, uint64_t n_words, uint64_t* second, uint64_t n_second_words);

/* Queries of the counted table.  The reference has no counterpart: its table is only ever
 * walked by the writers (kmer_hash_table.cpp:4318-4524); a caller that wants the count of a
 * k-mer or the abundance spectrum reads its output file back.  Here the full-key table in HBM
 * answers both.  A key's probe sequence ends at the first bucket with a free slot, so a lookup
 * is normally one 128-byte bucket read, present or absent.
 *   kc_lookup_device  T(c) of n_keys keys in device memory (kc_key_words() u64 each) into
 *                     dev_counts (uint32, 0 = absent).  key_layout KC_KEYS_DUMP: the kc_dump key
 *                     layout (word 0 most significant), either strand -- the k-mer is made
 *                     canonical first; a key with a bit set above bit 2k - 1 is not a k-mer and
 *                     answers 0.  KC_KEYS_TABLE: table keys as kc_route_device writes them (of a
 *                     context of the same k), looked up as they are; word 0 == 0 answers 0.
 *                     T(c) is kc_dump's: c mod 65536 for -m 0, min(c, 16383) otherwise; the
 *                     minimum abundance -a is NOT applied (as in kc_compact_lookup).  Follows the
 *                     *_device rule: enqueued on hip_stream after the work already queued there
 *                     and after the context's own queued work (staged host chunks are flushed
 *                     first); no host wait.
 *   kc_lookup         the same for host arrays; waits for the answer.
 *   kc_histogram      the count-of-counts of the whole table into hist[n_bins] (host array,
 *                     2 <= n_bins <= 65537): hist[v] = k-mers with T(c) == v for v < n_bins - 1,
 *                     hist[n_bins - 1] = k-mers with T(c) >= n_bins - 1 (hist[0]: only -m 0
 *                     counts that wrapped to a multiple of 65536).  Not filtered by -a.  One
 *                     sweep of the table; waits for the answer.
 * Any table answers (Bloom-gated, filled by merges or kc_insert_*, counted over several
 * batches); a table emptied by kc_reset or kc_clear_table answers 0 everywhere.  KC_ERR_STATE
 * without a table (a Bloom context before kc_bloom_finalize); n_keys = 0 is KC_OK.  No counter
 * of kc_stats changes. */
#define KC_KEYS_DUMP  0   /* kc_dump key layout, either strand */
#define KC_KEYS_TABLE 1   /* kc_route_device's table keys */
int kc_lookup_device(kc_ctx* ctx, const uint64_t* dev_keys, uint64_t n_keys, int key_layout, uint32_t* dev_counts,
                     void* hip_stream);
int kc_lookup(kc_ctx* ctx, const uint64_t* keys, uint64_t n_keys, int key_layout, uint32_t* counts);
int kc_histogram(kc_ctx* ctx, uint64_t* hist, uint32_t n_bins);

/* Sequence queries of the counted table: how abundant are the k-mers of this read, contig or
 * gene in what was counted.  One fused pass goes from text to a count per position -- no key is
 * written to or read back from HBM -- and a segmented reduction gives per-sequence statistics.
 *   kc_text_counts_device  The text is ONE byte stream of n_bytes in device memory, at any byte
 *                     address.  A, C, G, T in either case are bases; every other byte (N, a
 *                     newline, '>', ...) is a break.  dev_counts[p] (uint32, all n_bytes entries
 *                     are written) is T(c) of the canonical k-mer of text[p .. p + k) when all k
 *                     bytes are bases and p + k <= n_bytes, and KC_NO_KMER otherwise.  T(c) is
 *                     kc_lookup's: c mod 65536 for -m 0, min(c, 16383) otherwise, 0 if absent;
 *                     the minimum abundance -a is NOT applied.  Nothing is parsed: headers and
 *                     quality lines are the caller's to leave out, and sequence boundaries are
 *                     whatever break bytes the caller put between sequences (two sequences joined
 *                     with no break byte between them share the k - 1 windows across the joint).
 *   kc_text_counts    the same for host arrays; waits for the answer.
 *   kc_seq_stats_device  per-sequence statistics of the same kind of text.  offsets is a HOST
 *                     array of n_seqs + 1 non-decreasing byte offsets with offsets[n_seqs] <=
 *                     n_bytes (like the kc_chunk table beside a device image; copied before the
 *                     call returns); sequence i is the bytes [offsets[i], offsets[i + 1]).  Its
 *                     windows are the positions p in that range with p + k <= offsets[i + 1] and a
 *                     valid k-mer at p, so a window never spans two sequences, even when they are
 *                     adjacent with no break byte.  dev_stats[i] (device memory, n_seqs entries)
 *                     receives the kc_seq_stat below.  The per-position counts are scratch of the
 *                     context: the text runs in passes cut at sequence boundaries of at most the
 *                     context's staging batch (kc_config.batch_bytes) each, a longer single
 *                     sequence being a pass of its own length (4.4 bytes of scratch per byte).
 *                     Offsets that decrease or pass n_bytes: KC_ERR_ARG.
 *   kc_seq_stats      the same for a host text and a host result array; waits for the answer.
 * The *_device forms follow the *_device rule as kc_lookup_device does (enqueued on hip_stream
 * after the work queued there and after the context's own; no host wait beyond an earlier call's
 * offsets copy).  Any table answers, an emptied one 0 everywhere; KC_ERR_STATE without a table;
 * n_bytes = 0 and n_seqs = 0 are KC_OK; no counter of kc_stats changes. */
#define KC_NO_KMER 0xFFFFFFFFu      /* no k-mer starts at this position */
typedef struct {                    /* 32 bytes */
    uint32_t windows;   /* positions of the sequence where a k-mer starts (k bases, inside the sequence) */
    uint32_t present;   /* of those, T(c) >= 1 */
    uint32_t solid;     /* of those, T(c) >= solid_min */
    uint32_t min, median, max;  /* of T(c) over the windows, absent k-mers counting as 0; the median is
                                   element (windows - 1) / 2 of the sorted values (the lower median) */
    uint64_t sum;       /* sum of T(c) over the windows */
} kc_seq_stat;          /* windows == 0: every field 0 */
int kc_text_counts_device(kc_ctx* ctx, const uint8_t* dev_text, uint64_t n_bytes, uint32_t* dev_counts,
                          void* hip_stream);
int kc_text_counts(kc_ctx* ctx, const uint8_t* text, uint64_t n_bytes, uint32_t* counts);
int kc_seq_stats_device(kc_ctx* ctx, const uint8_t* dev_text, uint64_t n_bytes, const uint64_t* offsets,
                        uint64_t n_seqs, uint32_t solid_min, kc_seq_stat* dev_stats, void* hip_stream);
int kc_seq_stats(kc_ctx* ctx, const uint8_t* text, uint64_t n_bytes, const uint64_t* offsets, uint64_t n_seqs,
                 uint32_t solid_min, kc_seq_stat* stats);

/* Read correction: repair isolated base errors of a text from the counted table (spectrum-based
 * correction), in one device pass -- no count and no substituted k-mer crosses to the host.  The
 * text, the offsets and solid_min are those of kc_seq_stats*; s = max(solid_min, 1); T is
 * kc_lookup's count (-a is not applied).  For sequence i = bytes [a, b):
 *   windows      w with a <= w, w + k <= b and text[w .. w + k) all bases (never across two
 *                sequences, even when they are adjacent with no break byte);
 *   C(p)         the windows that hold position p: w <= p < w + k;
 *   candidate(p) text[p] is a base, C(p) is not empty and every window of C(p) has T < s;
 *   works(p, y)  y one of the three other bases: every window of C(p), with byte p replaced by y,
 *                has T >= s;
 *   accepted(p)  candidate(p) and exactly one y works;  ambiguous(p): two or three work;
 *   dropped(p)   accepted(p) and another accepted q of the same sequence has |p - q| < k (all
 *                such positions are dropped: no window of the output holds two changes).
 * out[p] is the working y in the letter case of text[p] when p is accepted and not dropped; every
 * other byte of the n_bytes is copied unchanged (breaks and the bytes outside [offsets[0],
 * offsets[n_seqs]) too).  Everything is evaluated on the ORIGINAL text and the unchanged table, so
 * the result does not depend on any order.  It follows that every window of the output that holds
 * a changed byte has T >= s, and every other window is the input's.
 *   kc_correct_device  dev_out receives all n_bytes; dev_out == dev_text (in place) is allowed,
 *                     any other overlap is KC_ERR_ARG.  dev_stats (device memory, n_seqs entries,
 *                     may be NULL) receives the kc_correct_stat below.  The text runs in passes cut
 *                     at sequence boundaries of at most the context's staging batch
 *                     (kc_config.batch_bytes) each, a longer single sequence being a pass of its own
 *                     length.  Scratch of the context per text byte of a pass: 3/8 byte of packed
 *                     stream, 4 bytes of per-position counts and 1 verdict byte (5.4 bytes; no
 *                     candidate list is kept: the kernels find the candidates in the verdict bytes).
 *   kc_correct        the same for host arrays (out == text allowed); waits for the answer.
 * The *_device form follows the *_device rule exactly as kc_seq_stats_device does (no host wait
 * beyond an earlier call's offsets copy); the argument and state errors are those of
 * kc_seq_stats*, and a NULL text or out with n_bytes > 0 is KC_ERR_ARG.  Any table answers; an
 * emptied one gives out == text with every base position that has covering windows a candidate.
 * n_bytes = 0 and n_seqs = 0 are KC_OK; no counter of kc_stats changes, the table is only read. */
typedef struct {            /* 16 bytes */
    uint32_t candidates;    /* candidate positions */
    uint32_t corrected;     /* accepted and not dropped: the bytes of the sequence that changed */
    uint32_t ambiguous;     /* candidates with two or three working bases */
    uint32_t dropped;       /* accepted positions closer than k to another accepted one */
} kc_correct_stat;          /* a sequence without windows: every field 0 */
int kc_correct_device(kc_ctx* ctx, const uint8_t* dev_text, uint64_t n_bytes, const uint64_t* offsets,
                      uint64_t n_seqs, uint32_t solid_min, uint8_t* dev_out, kc_correct_stat* dev_stats,
                      void* hip_stream);
int kc_correct(kc_ctx* ctx, const uint8_t* text, uint64_t n_bytes, const uint64_t* offsets, uint64_t n_seqs,
               uint32_t solid_min, uint8_t* out, kc_correct_stat* stats);

/* Table algebra: relate two counted tables in HBM.  The reference has no counterpart -- it counts
 * one input into one table, and its users join output files (k-mers of the child absent from the
 * mother, k-mers two runs share, a sample minus an adapter set, Jaccard similarity, the union of
 * several runs).  One fused kernel sweeps a's table, looks every key up in b's and adds the
 * operation's result into dst's table: no key or record goes through HBM between the three, and
 * nothing crosses to the host.  The UNION operations run it a second time over b for the keys a
 * lacks.  The result is itself a counted table: kc_write, kc_output_digest, kc_histogram,
 * kc_lookup*, kc_seq_stats*, kc_compact and a further kc_table_op work on dst unchanged.
 *   kc_table_op_device  dst += op(a, b).
 *     Counts are the RAW counts of the slots, the counts kc_route_table_device and
 *     kc_insert_counts_device move; T(c) is not applied to them, dst applies its own -m when it is
 *     read.  So in -m 1/2 min, max and sum saturate AFTER the operation: KC_OP_COUNTS_SUBTRACT of
 *     k-mers counted 20000 and 17000 times reads back 3000, KC_OP_INTERSECT_SUM of them 16383.
 *     A key of a is "in a" when a_min <= T(c) <= a_max, T(c) being the count kc_lookup reports for
 *     it in a's own mode (c mod 65536 for -m 0, min(c, 16383) otherwise); the same for b with
 *     b_min / b_max.  A min of 0 means 1, a max of 0 no upper bound.  A key outside its table's
 *     range counts as absent from that table.  The minimum abundance -a is applied nowhere.
 *     The results are ADDED into dst's table, as kc_insert_counts_device adds records: a dst
 *     fresh from kc_create, kc_reset or kc_clear_table holds exactly the result, repeated calls
 *     accumulate (the union of many tables, one call each).  dst's counters change as they do for
 *     kc_insert_counts_device (kc_stats.inserted += the counts added); a result that does not
 *     fit dst's table makes kc_finish on dst return KC_ERR_TABLE_FULL.  a's and b's tables and
 *     kc_stats do not change; dst may have any table size, and so may a and b (a table's keys do
 *     not depend on its geometry), any mode, and a or b may be Bloom-gated.
 *     dst == NULL inserts nothing and fills only the statistics; with a UNION operation that is
 *     the comparison of two samples: Jaccard = both / (a_keys + b_only), containment of a in b =
 *     both / a_keys.  dev_stats (device memory, may be NULL) is zeroed and filled by the call.
 *     a == b is allowed.  KC_ERR_ARG: dst equal to a or b, contexts of different k or device, an
 *     unknown op, reserved != 0, a min above a non-zero max, a NULL a, b or op.  KC_ERR_STATE: one
 *     of the three without a table (a Bloom context before kc_bloom_finalize) or with a job a
 *     failed pass left incomplete.  An a or b emptied by kc_reset or kc_clear_table holds no key.
 *     The message of a failed call is on dst (kc_last_error), on a when dst is NULL.
 *     Follows the *_device rule for ALL THREE contexts: the staged host chunks of each are
 *     flushed first, the work runs on hip_stream after what is queued there and after each
 *     context's own stream, and each context's later work follows it; no host wait (unless dst
 *     holds a compact representation, which is dropped: it is a snapshot of the table before).
 *   kc_table_op         the same with the statistics in host memory (may be NULL); waits. */
#define KC_OP_INTERSECT_MIN   0  /* keys in both;            min(ca, cb) */
#define KC_OP_INTERSECT_SUM   1  /* keys in both;            ca + cb     */
#define KC_OP_INTERSECT_LEFT  2  /* keys in both;            ca          */
#define KC_OP_SUBTRACT        3  /* keys of a not in b;      ca          */
#define KC_OP_COUNTS_SUBTRACT 4  /* keys of a; ca - cb where positive (cb = 0 if absent), else dropped */
#define KC_OP_UNION_SUM       5  /* keys in either;          ca + cb     */
#define KC_OP_UNION_MAX       6  /* keys in either;          max(ca, cb) */
typedef struct {            /* 24 bytes */
    int32_t  op;
    uint32_t a_min, a_max;  /* a key of a is "in a" when a_min <= T(c) <= a_max; a_min 0 means 1, a_max 0 = no upper bound */
    uint32_t b_min, b_max;  /* the same for b */
    uint32_t reserved;      /* 0 */
} kc_op_desc;
typedef struct {            /* 40 bytes */
    uint64_t a_keys;   /* keys in a (inside its range) */
    uint64_t both;     /* of those, in b (inside its range) */
    uint64_t b_only;   /* keys in b and not in a -- UNION ops only (the only ones that sweep b), else 0 */
    uint64_t out_keys; /* records the operation yields (added to dst when dst != NULL) */
    uint64_t out_sum;  /* sum of their counts */
} kc_op_stats;
int kc_table_op_device(kc_ctx* dst, kc_ctx* a, kc_ctx* b, const kc_op_desc* op, kc_op_stats* dev_stats,
                       void* hip_stream);
int kc_table_op(kc_ctx* dst, kc_ctx* a, kc_ctx* b, const kc_op_desc* op, kc_op_stats* stats);

/* The de Bruijn graph of the counted table: what comes next.  A counted k-mer set IS a de Bruijn
 * graph, and assembly, tip and bubble statistics, seed extension and repeat detection ask it for a
 * k-mer's neighbours; the reference's users rebuild a hash table from the output text for that.
 * Here the table's keys give their k-mers back, every neighbour is one probe, and no key leaves HBM.
 * Strings are over ACGT with codes A 0, C 1, G 2, T 3; rc is the reverse complement, canon(z) =
 * min(z, rc(z)); T is kc_lookup's count (-a is applied nowhere).  A range is min_count (0 means 1)
 * and max_count (0 = no upper bound), as in kc_op_desc.
 *   node          a canonical k-mer c the table holds with min_count <= T(c) <= max_count.
 *   edges of c    8 bits: bit y is set when canon(c[1:] + y) is a node (side R), bit 4 + y when
 *                 canon(y + c[:-1]) is a node (side L); deg_R and deg_L are the popcounts of the
 *                 two nibbles.  (c may be its own neighbour: AAA...A, a hairpin x -> rc(x).)
 *   facing side   side R, z = c[1:] + y, d = canon(z): c sits on d's side L if d == z, else on d's
 *                 side R; side L, z = y + c[:-1]: on d's side R if d == z, else on d's side L.
 *   link(c, s)    deg_s(c) == 1, its one neighbour d != c, neither c nor d is its own reverse
 *                 complement (even k only), and the degree of d's facing side is 1.  Links are
 *                 mutual: link(c, s) holds exactly when link(d, facing side) does, and that one
 *                 leads back to (c, s).  Every maximal path of links is a unitig; the non-circular
 *                 unitigs number nodes - link_ends / 2.
 *   flags         16 bits per node: bits 0-7 the edges, KC_GRAPH_LINK_R, KC_GRAPH_LINK_L,
 *                 KC_GRAPH_NODE (always set); every other bit 0.
 *   kc_neighbors_device  counts[8 i + y] = T(canon(x[1:] + y)), counts[8 i + 4 + y] =
 *                 T(canon(y + x[:-1])), 0 = absent, x = key i (kc_key_words() words each).
 *                 KC_KEYS_DUMP: x is the k-mer as given -- the strand is respected, so the other
 *                 strand's answer has R and L swapped and complemented; a key with a bit above
 *                 2k - 1 answers eight zeros.  KC_KEYS_TABLE: x is the canonical k-mer the table
 *                 key encodes; word 0 == 0 answers zeros.  No range is applied.
 *   kc_neighbors  the same for host arrays; waits for the answer.
 *   kc_graph_device  one record per node, kc_key_words() + 1 words: the key in kc_dump's layout,
 *                 then T(c) | (uint64_t)flags << 32; the record order is unspecified, like
 *                 kc_write's lines.  dev_records == NULL gives the statistics only.
 *                 *dev_n_records is always the number of nodes; only the first `capacity` records
 *                 are written and nothing is written past them (kc_stats.distinct always suffices
 *                 as capacity).  dev_stats and dev_n_records (device memory) may be NULL.  Two
 *                 sweeps of the table: the first probes every node's eight neighbours and keeps one
 *                 edge byte per table slot in scratch of the context (kc_stats.table_slots bytes),
 *                 the second finds the links from those bytes, reduces the statistics and appends
 *                 the records.
 *   kc_graph      the same with the records (free with kc_free) and the statistics in host
 *                 memory; records, n_records and stats may each be NULL (records == NULL or
 *                 n_records == NULL: statistics only); waits.
 * The *_device forms follow the *_device rule as kc_lookup_device does: staged host chunks are
 * flushed first, the work runs on hip_stream after what is queued there and after the context's
 * own stream, and the context's later work follows it; no host wait (the first kc_graph_device on a
 * table allocates the edge scratch).  An emptied table (kc_reset, kc_clear_table) has no nodes and
 * kc_neighbors* answers zeros.  KC_ERR_STATE: no table (a Bloom context before kc_bloom_finalize)
 * or a job a failed pass left incomplete.  KC_ERR_ARG: k < 2, min_count above a non-zero max_count,
 * a NULL key or count array with n_keys > 0, an unknown layout.  n_keys == 0 is KC_OK.  Any table
 * answers: Bloom-gated, merged, counted by a deferred level 3, any mode.  The table is only read
 * and no counter of kc_stats changes. */
#define KC_GRAPH_EDGE_R(y) (1u << (y))        /* canon(c[1:] + y) is a node */
#define KC_GRAPH_EDGE_L(y) (1u << (4 + (y)))  /* canon(y + c[:-1]) is a node */
#define KC_GRAPH_LINK_R 0x0100u  /* link(c, R) */
#define KC_GRAPH_LINK_L 0x0200u  /* link(c, L) */
#define KC_GRAPH_NODE   0x8000u  /* set in every record */
typedef struct {          /* 80 bytes */
    uint64_t nodes;           /* nodes */
    uint64_t edge_ends;       /* set edge bits (an edge between two nodes counts at both ends) */
    uint64_t link_ends;       /* set link bits (even: links are mutual) */
    uint64_t isolated;        /* nodes with both degrees 0 */
    uint64_t palindromes;     /* nodes with c == rc(c) */
    uint64_t side_degree[5];  /* node sides with degree 0..4; sums to 2 * nodes */
} kc_graph_stats;
int kc_neighbors_device(kc_ctx* ctx, const uint64_t* dev_keys, uint64_t n_keys, int key_layout,
                        uint32_t* dev_counts /* 8 per key */, void* hip_stream);
int kc_neighbors(kc_ctx* ctx, const uint64_t* keys, uint64_t n_keys, int key_layout, uint32_t* counts);
int kc_graph_device(kc_ctx* ctx, uint32_t min_count, uint32_t max_count, uint64_t* dev_records, uint64_t capacity,
                    uint64_t* dev_n_records, kc_graph_stats* dev_stats, void* hip_stream);
int kc_graph(kc_ctx* ctx, uint32_t min_count, uint32_t max_count, uint64_t** records, uint64_t* n_records,
             kc_graph_stats* stats);

/* The unitigs of that graph: the sequences the link bits spell.  Compacted unitigs are what
 * assemblers, variant callers and colored-graph indexers read, what BCALM and GGCAT write, and the
 * compact lossless form of the k-mer set: nodes + (k - 1) * unitigs bases instead of k * nodes.  All
 * terms are kc_graph_device's: node, range, side, facing side, link(c, s).
 *   unitig        a maximal path of links c_0 ... c_{n-1}, each node read on one strand, x_i in
 *                 {c_i, rc(c_i)} with x_{i+1}[:-1] == x_i[1:]; its string is x_0 followed by the last
 *                 character of each later x_i, n + k - 1 bases over ACGT.  Every node lies in exactly
 *                 one unitig; a node without links is a unitig of one node.
 *   strand        unspecified: either of the two strings of a unitig is a right answer (a one-node
 *                 unitig may be c or rc(c)).
 *   circular      the link at the far side of c_{n-1} leads back to c_0 (then n >= 2).  It is
 *                 written as the same n + k - 1 bases starting at an unspecified node, so its last
 *                 k - 1 bases repeat its first k - 1, and it is flagged KC_UNITIG_CIRCULAR.
 *   states        the method rests on the directed states (node, exit side): next(c, s) = (d, the
 *                 other side of d's facing side) when link(c, s) holds, nothing otherwise.  next is
 *                 injective and rev(c, s) = (c, 1 - s) reverses it; self-links are excluded by the
 *                 link rule, so the states form disjoint paths and cycles, each unitig is two paths
 *                 or two cycles that mirror each other, and no path passes one node twice.  Paths
 *                 are ranked by pointer jumping in ceil(log2(longest path)) rounds; nothing walks a
 *                 unitig node by node.
 *   kc_unitigs_device  one kc_unitig per unitig and its bases (ASCII ACGT, one byte each) at
 *                 dev_bases + offset.  Record order and offset order are unspecified, as kc_graph's
 *                 record order is.  The offsets are distinct, non-overlapping places in [0,
 *                 stats.bases), handed out whatever the capacities are; record i is written only
 *                 when i < cap_unitigs, a unitig's bases only when offset + n_nodes + k - 1 <=
 *                 cap_bases, and nothing is written past either capacity.  *dev_stats always holds
 *                 the full totals, so a statistics-only call sizes a second one.  dev_unitigs,
 *                 dev_bases and dev_stats (device memory) may each be NULL.
 *   kc_unitigs    the same in host memory of the exact size (free both with kc_free); any of the
 *                 three out-pointers may be NULL; waits.  The ranking runs once: rank, read the
 *                 totals, allocate, write.
 * kc_unitigs_device follows the *_device rule as kc_graph_device does: staged host chunks are
 * flushed first, the work runs on hip_stream after what is queued there and after the context's own
 * stream, and the context's later work follows it; no host wait -- the number of jump launches is
 * fixed by the host, ceil(log2(2 * ids)) + 1 for each of the two rankings (the second ranks the
 * circles, cut at their least node), and a launch whose predecessor moved no state returns at once.
 * Errors are kc_graph's: KC_ERR_ARG for k < 2 or min_count above a non-zero max_count, KC_ERR_STATE
 * without a table or after a failed pass, KC_ERR_NOMEM when the scratch does not fit -- reported
 * before any kernel of kc_unitigs_device is launched; kc_unitigs first runs and waits for the
 * count-only sweep that sizes the scratch, and reports it before any kernel of the ranking; an
 * emptied table gives zero unitigs.  The table is only read and
 * no counter of kc_stats changes.
 * Scratch of the context (grows only, shared with kc_graph's edge bytes): 5 bytes per table slot
 * (kc_stats.table_slots: the edge byte, the slot's node id) and 140 bytes per node id -- two states
 * of 24 bytes in each of two buffers, two successors, T(c), the slot, and the unitig's start,
 * position, offset and length.  kc_unitigs counts the k-mers with T(c) >= min_count first and has
 * that many ids (>= the nodes); kc_unitigs_device cannot wait for a count and has table_slots ids:
 *   scratch = 5 * table_slots + 140 * ids bytes,  ids < 2^30 (else KC_ERR_NOMEM).
 * The kernels work on the nodes there are, whatever the ids allocated. */
#define KC_UNITIG_CIRCULAR 1u  /* kc_unitig.flags: the unitig is circular */
typedef struct {            /* 32 bytes */
    uint64_t offset;        /* of its first base, counted in an unbounded bases buffer */
    uint64_t n_nodes;       /* its string has n_nodes + k - 1 bases */
    uint64_t count_sum;     /* sum of T(c) over its nodes (mean abundance = count_sum / n_nodes) */
    uint64_t flags;         /* KC_UNITIG_CIRCULAR 1; every other bit 0 */
} kc_unitig;
typedef struct {            /* 40 bytes */
    uint64_t unitigs, circular, nodes, bases, max_nodes;   /* bases = nodes + (k-1)*unitigs; max_nodes = longest unitig */
} kc_unitig_stats;
int kc_unitigs_device(kc_ctx* ctx, uint32_t min_count, uint32_t max_count, kc_unitig* dev_unitigs, uint64_t cap_unitigs,
                      uint8_t* dev_bases, uint64_t cap_bases, kc_unitig_stats* dev_stats, void* hip_stream);
int kc_unitigs(kc_ctx* ctx, uint32_t min_count, uint32_t max_count, kc_unitig** unitigs, uint8_t** bases,
               kc_unitig_stats* stats);   /* kc_free both */

/* The compacted de Bruijn graph: the unitigs and the edges between them, what BCALM, GGCAT and
 * Bifrost write as GFA -- segments and their overlaps of k - 1 bases.  All terms are
 * kc_graph_device's and kc_unitigs_device's: node, range, side, facing side, link(c, s), unitig,
 * circular.
 *   orientation   a unitig record U has the string S_U the same call wrote; U+ is S_U, U- is rc(S_U).
 *   palindromic unitig  S_U == rc(S_U).  The link rule excludes palindromes, so it is a unitig of one
 *                 node that is its own reverse complement (even k only).  It has one orientation,
 *                 always written +.
 *   unitig end    a pair (node c, side s) with link(c, s) false.  An open unitig has two ends -- of a
 *                 palindromic one only side R counts -- and a circular unitig has none.
 *   edge          one per set edge bit of a unitig end (c, s): d the neighbour, t the side of d that c
 *                 sits on (the facing side), U the unitig of c and V the unitig of d.
 *                 from_rev = 0 when U is left through the end of S_U: the reading of c when left
 *                 through s (c for R, rc(c) for L) is c's reading inside S_U; else 1.
 *                 to_rev = 0 when V is entered at the start of S_V: d entered through t (d for t = L,
 *                 rc(d) for t = R) is d's reading inside S_V; else 1.
 *                 Both bits are 0 for a palindromic unitig, and side L of a palindromic node reports
 *                 nothing: its neighbours are the ones on its side R.
 *   properties    the last k - 1 bases of orient(S_U, from_rev) are the first k - 1 of orient(S_V,
 *                 to_rev).  The tuples (from, from_rev, to, to_rev) are distinct.  Every edge's mirror
 *                 (to, !to_rev, from, !from_rev) is in the list (a palindromic unitig's bit stays 0):
 *                 a hairpin (U, a, U, !a) is its own mirror and appears once, a homopolymer gives
 *                 (U, +, U, +) and (U, -, U, -).  edges == kc_graph_stats.edge_ends - link_ends - the
 *                 edge ends on side L of palindromic nodes.  A circle's closing link is a link, not
 *                 an edge: KC_UNITIG_CIRCULAR says it, the list does not.
 *   kc_unitig_graph_device  unitigs and bases as kc_unitigs_device writes them, capacity rules
 *                 included (offsets and record indices are handed out whatever the capacities are).
 *                 Edge j is written only when j < cap_edges, nothing past it; the edge order is
 *                 unspecified.  from and to are record indices of this same call's kc_unitig records
 *                 in their unbounded numbering -- valid numbers also where cap_unitigs cut the
 *                 records -- and fit 32 bits because ids < 2^30.  *dev_stats always holds the full
 *                 totals, so a statistics-only call sizes the next one.  dev_unitigs, dev_bases,
 *                 dev_edges and dev_stats (device memory) may each be NULL; dev_edges is 16-byte
 *                 aligned, as every device allocation is (else KC_ERR_ARG).
 *   kc_unitig_graph  the same in host memory of the exact size (free all three with kc_free); any of
 *                 the four out-pointers may be NULL; waits.  The ranking runs once: rank, read the
 *                 totals (records and edges counted without buffers), allocate, write.
 * The *_device rule, the errors, KC_ERR_NOMEM before any kernel of the call and the emptied table
 * (zero unitigs, zero edges) are kc_unitigs*'s; kc_unitig_graph_device has no host wait.  The table
 * is only read and no counter of kc_stats changes.  Two kernels follow kc_unitigs_device's: the
 * records' kernel also leaves each unitig's record index at its first node's id, and one more pass
 * over the node ids counts the edge bits of every unitig end (no probe) and, with dev_edges, probes
 * each edge's neighbour once for its slot, hence its unitig.  That index costs 4 bytes per id, which
 * only these two calls allocate:
 *   scratch = 5 * table_slots + 144 * ids bytes,  ids as for kc_unitigs* (< 2^30, else KC_ERR_NOMEM). */
#define KC_EDGE_FROM_REV 1u  /* kc_unitig_edge.flags: the edge leaves `from` through the start of its string */
#define KC_EDGE_TO_REV   2u  /* kc_unitig_edge.flags: the edge enters `to` at the end of its string */
typedef struct {            /* 16 bytes */
    uint32_t from, to;      /* record indices of this call's kc_unitig records */
    uint32_t flags;         /* KC_EDGE_FROM_REV | KC_EDGE_TO_REV; every other bit 0 */
    uint32_t reserved;      /* 0 */
} kc_unitig_edge;
typedef struct {            /* 64 bytes */
    uint64_t unitigs, circular, nodes, bases, max_nodes;   /* as kc_unitig_stats */
    uint64_t edges;         /* edge records */
    uint64_t dead_ends;     /* unitig ends without any edge */
    uint64_t reserved;      /* 0 */
} kc_cdbg_stats;
int kc_unitig_graph_device(kc_ctx* ctx, uint32_t min_count, uint32_t max_count, kc_unitig* dev_unitigs,
                           uint64_t cap_unitigs, uint8_t* dev_bases, uint64_t cap_bases, kc_unitig_edge* dev_edges,
                           uint64_t cap_edges, kc_cdbg_stats* dev_stats, void* hip_stream);
int kc_unitig_graph(kc_ctx* ctx, uint32_t min_count, uint32_t max_count, kc_unitig** unitigs, uint8_t** bases,
                    kc_unitig_edge** edges, kc_cdbg_stats* stats);   /* kc_free all three */

/* Read paths: where every sequence of a text lies in the compacted graph -- what SPAdes, MEGAHIT and
 * Velvet thread reads through the graph for, what Bifrost and pufferfish answer per k-mer (which
 * unitig, which offset, which strand), what GraphAligner and Bandage read as GAF beside the GFA.
 * Record indices differ from launch to launch, so a path can only name the unitigs of the call that
 * wrote them: one call writes graph and paths together.  All terms of kc_graph_device,
 * kc_unitigs_device, kc_unitig_graph_device and kc_seq_stats_device hold: node, range, unitig, S_U,
 * orientation (orient(S_U, 0) = S_U, orient(S_U, 1) = rc(S_U)), palindromic unitig, circular, the
 * text and its break bytes, the offsets array, a sequence's windows (never spanning two sequences).
 *   located window  a window at text position p whose canonical k-mer is a node of the range.  Its
 *                 place is (U, rev, q): U the record index of the node's unitig; rev = 0 when the
 *                 window's k bases, upper-cased, read as the node reads inside S_U, else 1 (always 0
 *                 on a palindromic unitig); q the index of that k-mer in orient(S_U, rev), so
 *                 orient(S_U, rev)[q .. q + k) equals the window's bases.
 *   run           a maximal set of windows at consecutive positions p, p + 1, ... of one sequence,
 *                 all located on the same U with the same rev, whose q grows by one per window; on
 *                 a circular unitig q steps from n_nodes - 1 to 0, so a run may go round a circle
 *                 any number of times and `windows` may exceed n_nodes.  The rule is arithmetic on
 *                 (U, rev, q), the unitig's n_nodes and its circular flag; nothing is probed twice.
 *   joined        a run is joined when the window at p - 1 of the same sequence is located too (it
 *                 belongs to the run before).  A chain is a maximal sequence of runs each joined to
 *                 the one before: a maximal stretch of consecutive located windows.
 *   properties    a joined run starts at q = 0, and the run before it ends at the last k-mer of its
 *                 oriented unitig.  For two such runs (U, a) then (V, b) the tuple (U, a, V, b) is in
 *                 the same call's edge list (a palindromic unitig's bit reads 0 there), except U == V
 *                 circular with a == b, which the run rule has merged already.  No run on a circular
 *                 unitig is joined or followed by a joined run.  Along a chain the text equals the
 *                 walk's string.
 *   kc_read_paths_device  the graph part is kc_unitig_graph_device's, unchanged in every rule and run
 *                 by the same host code.  The text part runs after the call's last records launch,
 *                 whose numbering the caller receives.  dev_text, n_bytes, offsets (HOST array of
 *                 n_seqs + 1 entries) and n_seqs are kc_seq_stats_device's.  Runs are written in
 *                 ascending text_pos order -- hence sequence by sequence; this order is specified,
 *                 unlike the records' and the edges'.  Run j is written only when j < cap_runs and
 *                 nothing past it; *dev_path_stats, and first_run and runs of every kc_path_seq, hold
 *                 the full totals whatever the capacity, so a statistics-only call sizes the next.
 *                 `unitig` is a valid number of the unbounded record numbering even where
 *                 cap_unitigs cut the records.  Every output pointer may be NULL; dev_edges and
 *                 dev_runs are 16-byte aligned, as every device allocation is (else KC_ERR_ARG).  The
 *                 text runs in passes cut at sequence boundaries of at most kc_config.batch_bytes,
 *                 a longer single sequence being a pass of its own; the run numbering carries from
 *                 pass to pass on the device.  No host wait beyond an earlier call's offsets copy.
 *   kc_read_paths  the same in host memory of the exact sizes (kc_free the five arrays); any
 *                 out-pointer may be NULL; waits.  The ranking runs once; the text part runs twice,
 *                 the first time without buffers for the number of runs.
 * The errors are kc_unitig_graph*'s and kc_seq_stats*'s; KC_ERR_NOMEM comes before any kernel of
 * the device form.  An emptied table gives zero unitigs and zero runs, every window unlocated;
 * n_bytes = 0 and n_seqs = 0 are KC_OK.  The table is only read and no counter of kc_stats changes.
 * Kernels: one fused pass from the packed text to a place per position (one probe and four gathers
 * per window, no key through HBM), then per tile of 256 positions the run heads, one workgroup's
 * scan of the tiles, and the emit, where every run's LAST window writes its record (the heads before
 * it number it, the last head before it starts it); the per-sequence sums are atomics per run, chain
 * and stretch of windows.  Scratch per pass, on top of kc_unitig_graph*'s:
 *   scratch = 5 * table_slots + 144 * ids + 8.5 * pass bytes,
 * 8 bytes of place and 3/8 byte of packed text per text byte and 32 bytes per 256; 32 bytes per
 * sequence of the text more when dev_seq is NULL. */
#define KC_RUN_REV    1u   /* kc_path_run.flags: the run reads its unitig as U- */
#define KC_RUN_JOINED 2u   /* kc_path_run.flags: the window before its first is located too */
#define KC_NO_UNITIG  0xFFFFFFFFu
typedef struct {            /* 32 bytes, written with 16-byte stores */
    uint64_t text_pos;      /* byte offset of the run's first window in the text */
    uint32_t seq;           /* index of its sequence */
    uint32_t windows;       /* consecutive window starts text_pos .. text_pos + windows - 1 */
    uint32_t unitig;        /* record index of this call's kc_unitig records */
    uint32_t pos;           /* q of the first window in orient(S_U, rev) */
    uint32_t flags;         /* KC_RUN_REV | KC_RUN_JOINED; every other bit 0 */
    uint32_t reserved;      /* 0 */
} kc_path_run;
typedef struct {            /* 32 bytes */
    uint64_t first_run;     /* index of the sequence's first run in the unbounded run numbering */
    uint32_t windows, located, runs, chains;
    uint32_t longest_chain; /* windows of its longest chain; == windows > 0: the sequence threads the graph whole */
    uint32_t reserved;      /* 0 */
} kc_path_seq;              /* a sequence without windows: first_run as defined, every other field 0 */
typedef struct {            /* 64 bytes */
    uint64_t seqs, windows, located, runs, chains;
    uint64_t threaded;      /* sequences with windows > 0 and longest_chain == windows */
    uint64_t reserved[2];   /* 0 */
} kc_path_stats;
int kc_read_paths_device(kc_ctx* ctx, uint32_t min_count, uint32_t max_count, kc_unitig* dev_unitigs,
                         uint64_t cap_unitigs, uint8_t* dev_bases, uint64_t cap_bases, kc_unitig_edge* dev_edges,
                         uint64_t cap_edges, kc_cdbg_stats* dev_cdbg_stats, const uint8_t* dev_text, uint64_t n_bytes,
                         const uint64_t* offsets, uint64_t n_seqs, kc_path_run* dev_runs, uint64_t cap_runs,
                         kc_path_seq* dev_seq, kc_path_stats* dev_path_stats, void* hip_stream);
int kc_read_paths(kc_ctx* ctx, uint32_t min_count, uint32_t max_count, kc_unitig** unitigs, uint8_t** bases,
                  kc_unitig_edge** edges, kc_cdbg_stats* cdbg_stats, const uint8_t* text, uint64_t n_bytes,
                  const uint64_t* offsets, uint64_t n_seqs, kc_path_run** runs, kc_path_seq** seq,
                  kc_path_stats* path_stats);   /* kc_free all five */

/* Graph cleaning: the graph of src's range without its short tips and its short isolated unitigs,
 * as a new counted table -- the step Bifrost (-i, -d), Minia, MEGAHIT and Velvet run on the raw
 * graph of sequencing reads before anything else.  All terms are kc_graph_device's and
 * kc_unitig_graph_device's: node, range [min_count, max_count], side, edge bits, link, unitig,
 * circular, unitig end.
 *   degree        of an end of a unitig U of the range's graph: the popcount of the edge nibble of
 *                 the end's node at the end's side.  Edge bits only count neighbours that are nodes
 *                 of the range.  An open unitig has two ends; for n = 1 they are the two sides of
 *                 its one node.
 *   isolated      U is open and both ends have degree 0.
 *   tip           U is open and exactly one end has degree 0.  A circular unitig is neither.
 *   palindromes   no special case: a palindromic node's side-L neighbours are its side-R neighbours
 *                 complemented, so its two nibbles have equal popcounts.  It can be isolated and can
 *                 never be a tip.
 *   self edges    the rule reads the edge bits alone: an end whose only edge leads back into U -- a
 *                 hairpin, a homopolymer's self loop -- counts as connected.
 *   guard         with max_mean != 0, U is removable only when count_sum(U) <= (uint64_t)max_mean * n
 *                 (count_sum: kc_unitig.count_sum, the sum of T(c) over U's n nodes).
 *   removal       U is removed when it is a tip, tip_max_nodes != 0, n <= tip_max_nodes and the guard
 *                 passes, or when it is isolated, iso_max_nodes != 0, n <= iso_max_nodes and the guard
 *                 passes.  0 switches a rule off; the customary value of both is k - 1 (Bifrost's
 *                 -i -d: tips and isolated unitigs shorter than k k-mers).
 *   order         every verdict is taken on the original graph, so all removals are simultaneous and
 *                 the result depends on no order.  One consequence is left as it is: at a junction
 *                 all of whose branches are short tips, all of them go.  Removing tips makes new,
 *                 longer unitigs and sometimes new tips: rounds compose by calling it again on dst.
 *   kept nodes    every node of a unitig that is not removed.  Each kept node's raw count (the
 *                 slot's count, not T(c)) is added into dst exactly as kc_table_op_device adds its
 *                 results: a fresh dst holds exactly the cleaned graph, repeated calls accumulate,
 *                 kc_stats.inserted grows by the counts added, a dst that is too small makes
 *                 kc_finish(dst) return KC_ERR_TABLE_FULL, and a compact snapshot of dst is dropped.
 *                 K-mers of src outside the range are not nodes and are not copied; with both rules
 *                 off the call copies the range's nodes.
 *   statistics    dst == NULL fills only the statistics: that call sizes a destination.  nodes ==
 *                 out_keys + tip_nodes + isolated_nodes always.
 *   kc_clean_device  follows the *_device rule for both contexts as kc_table_op_device does and has
 *                 no host wait; its node ids are sized by src's table slots, as
 *                 kc_unitig_graph_device's.  dev_stats (device memory) may be NULL.
 *   kc_clean      counts the ids first (the k-mers with T(c) >= min_count), runs the ranking once and
 *                 waits for the answer; stats (host memory) may be NULL.
 * Errors: KC_ERR_ARG for dst == src, a different k or device, reserved != 0, min_count above a
 * non-zero max_count, k < 2, a NULL src or desc; KC_ERR_STATE when either context has no table or a
 * failed pass left it incomplete; KC_ERR_NOMEM when the scratch does not fit, reported before any
 * kernel of the call (kc_clean: of the ranking) is launched.  The message goes on dst, or on src when
 * dst is NULL.  An emptied src gives all-zero statistics and adds nothing.  src's table and kc_stats
 * never change.
 * Method: kc_unitigs_device's ranking and its records' kernel as they are, then one pass over the
 * node ids in which the node at position 0 of every unitig reads its two end states, tells open from
 * circular by their successors, reads the two ends' edge nibbles and writes the verdict at its id,
 * and one pass in which every kept node reads its slot's key and count word and inserts them into
 * dst.  The verdict costs one byte per id on top of kc_unitigs*'s scratch of src, which only these
 * two calls allocate:
 *   scratch = 5 * table_slots + 141 * ids bytes,  ids as for kc_unitigs* (< 2^30, else KC_ERR_NOMEM). */
typedef struct {            /* 24 bytes */
    uint32_t min_count, max_count;   /* the range, as kc_graph_device's */
    uint32_t tip_max_nodes;          /* 0: tips are kept */
    uint32_t iso_max_nodes;          /* 0: isolated unitigs are kept */
    uint32_t max_mean;               /* 0: no guard */
    uint32_t reserved;               /* 0 */
} kc_clean_desc;
typedef struct {            /* 64 bytes */
    uint64_t unitigs, nodes;         /* of the range's graph: kc_unitig_stats' */
    uint64_t tips, tip_nodes;        /* removed tips and their nodes */
    uint64_t isolated, isolated_nodes;   /* removed isolated unitigs and their nodes */
    uint64_t out_keys, out_sum;      /* kept nodes and the sum of their raw counts (added to dst when dst != NULL) */
} kc_clean_stats;
int kc_clean_device(kc_ctx* dst, kc_ctx* src, const kc_clean_desc* d, kc_clean_stats* dev_stats, void* hip_stream);
int kc_clean(kc_ctx* dst, kc_ctx* src, const kc_clean_desc* d, kc_clean_stats* stats);

/* Bubble popping: the graph of src's range without the weaker of its parallel unitigs, as a new
 * counted table -- the step that goes with tip clipping in Velvet (tour bus), Minia, MEGAHIT (merge
 * bubbles) and SPAdes (bulge remover).  A substitution in the middle of a read leaves a path of k
 * error k-mers beside the true path between the same two junctions, an indel one of about k - 1, a
 * heterozygous site two real paths.  All terms are kc_graph_device's, kc_unitig_graph_device's and
 * kc_clean_device's: node, range [min_count, max_count], side, edge bits, unitig, unitig end, degree
 * of an end, palindromic unitig, circular, edge (from, from_rev, to, to_rev).
 *   branch        U is a branch when it is open and not palindromic, both its ends have degree
 *                 exactly 1, and neither of its two edges leads to U itself.
 *   anchor        the unitig end that an end of a branch is attached to: for the edge (U, from_rev, V,
 *                 to_rev) the anchor is (V, 1 - to_rev), the from_rev value of the mirror edge.  A
 *                 palindromic V has one orientation, so its anchors all read (V, 1).  A branch has
 *                 two anchors; if they are the same unitig end, U is not a branch.  An anchor end
 *                 always has degree >= 2 (otherwise the link rule would have merged it), so an
 *                 anchor is never itself a branch through that end.
 *   parallel      two different branches with the same unordered pair of anchors.  At most four
 *                 branches share an anchor end.
 *   beats         U' beats U when count_sum(U') * n(U) > count_sum(U) * n(U'), compared exactly (the
 *                 products need more than 64 bits), or the two products are equal and name(U') <
 *                 name(U).  name(U) is the smaller of the canonical k-mer strings of U's two end
 *                 nodes, in A < C < G < T order, as kc_dump writes keys; distinct unitigs have
 *                 distinct names.
 *   popped        U is popped when max_nodes != 0 and n(U) <= max_nodes, the guard passes (max_mean
 *                 == 0 or count_sum(U) <= (uint64_t)max_mean * n(U)), and some branch U' exists that
 *                 is parallel to U, has n(U') <= max_nodes, has |n(U) - n(U')| <= max_diff, and
 *                 beats U.  max_diff = 0 means arms of equal length only (SNP bubbles); the
 *                 customary max_nodes is k.
 *   order         every verdict is taken on the one graph, so removals are simultaneous and depend
 *                 on no order.  In every set of mutually parallel branches, the one that no other
 *                 beats stays.  No anchor is removed.  Paths of more than one unitig (nested
 *                 bubbles) are not looked at; popping joins unitigs, so rounds compose by calling it
 *                 again on dst, and with kc_clean by calling one on the other's dst.
 *   kept nodes    every node of a unitig that is not popped.  Each kept node's raw count (the
 *                 slot's count, not T(c)) is added into dst exactly as kc_table_op_device adds its
 *                 results: a fresh dst holds exactly the popped graph, repeated calls accumulate,
 *                 kc_stats.inserted grows by the counts added, a dst that is too small makes
 *                 kc_finish(dst) return KC_ERR_TABLE_FULL, and a compact snapshot of dst is dropped.
 *                 K-mers of src outside the range are not nodes and are not copied; with max_nodes
 *                 == 0 the call copies the range's nodes.
 *   statistics    dst == NULL fills only the statistics: that call sizes a destination.  nodes ==
 *                 out_keys + popped_nodes always.
 *   kc_pop_bubbles_device  follows the *_device rule for both contexts as kc_table_op_device does and
 *                 has no host wait; its node ids are sized by src's table slots, as
 *                 kc_unitig_graph_device's.  dev_stats (device memory) may be NULL.
 *   kc_pop_bubbles  counts the ids first (the k-mers with T(c) >= min_count), runs the ranking once
 *                 and waits for the answer; stats (host memory) may be NULL.
 * Errors: KC_ERR_ARG for dst == src, a different k or device, reserved != 0, min_count above a
 * non-zero max_count, k < 2, a NULL src or desc; KC_ERR_STATE when either context has no table or a
 * failed pass left it incomplete; KC_ERR_NOMEM when the scratch does not fit, reported before any
 * kernel of the call (kc_pop_bubbles: of the ranking) is launched.  The message goes on dst, or on
 * src when dst is NULL.  An emptied src gives all-zero statistics and adds nothing.  src's table and
 * kc_stats never change.
 * Method: kc_unitigs_device's ranking and its records' kernel as they are, then one pass over the
 * node ids in which the node at position 0 of every unitig with two ends of degree 1 probes the one
 * neighbour of each end and leaves the two anchors -- 2 * the neighbour's node id + its facing side
 * -- at its id; one pass in which every branch walks the at most four edges of one of its anchor
 * ends, probes each neighbour, compares that unitig's anchors with its own and writes the verdict;
 * and kc_clean_device's copy of the kept nodes.  A branch costs at most six probes.  The anchors
 * cost 8 bytes per id on top of kc_clean*'s scratch of src, which only these two calls allocate:
 *   scratch = 5 * table_slots + 149 * ids bytes,  ids as for kc_unitigs* (< 2^30, else KC_ERR_NOMEM). */
typedef struct {            /* 24 bytes */
    uint32_t min_count, max_count;   /* the range, as kc_graph_device's */
    uint32_t max_nodes;     /* 0: nothing is popped, the call copies the range's nodes */
    uint32_t max_diff;      /* the most two arms' node counts may differ by; 0: equal lengths only */
    uint32_t max_mean;      /* 0: no guard */
    uint32_t reserved;      /* 0 */
} kc_bubble_desc;
typedef struct {            /* 64 bytes */
    uint64_t unitigs, nodes;        /* of the range's graph: kc_unitig_stats' */
    uint64_t branches;              /* unitigs that are branches */
    uint64_t parallel;              /* branches with at least one parallel branch, whatever the limits */
    uint64_t popped, popped_nodes;  /* popped branches and their nodes */
    uint64_t out_keys, out_sum;     /* kept nodes and the sum of their raw counts (added to dst when dst != NULL) */
} kc_bubble_stats;
int kc_pop_bubbles_device(kc_ctx* dst, kc_ctx* src, const kc_bubble_desc* d, kc_bubble_stats* dev_stats, void* hip_stream);
int kc_pop_bubbles(kc_ctx* dst, kc_ctx* src, const kc_bubble_desc* d, kc_bubble_stats* stats);

/* Weak-link removal: the graph of src's range without its short interior unitigs of low local
 * coverage, as a new counted table -- the third simplification that MEGAHIT (remove low local
 * coverage), SPAdes (low-coverage edge remover, erroneous-connection remover) and Velvet (coverage
 * cutoff) run beside tip clipping and bubble popping.  A chimeric read, or a stray path of error
 * k-mers that lands between two real paths, leaves a short unitig of count about 1 that is connected
 * at both ends: neither a tip nor isolated, and no bubble arm unless a parallel arm happens to exist.
 * All terms are kc_graph_device's, kc_unitig_graph_device's and kc_clean_device's: node, range
 * [min_count, max_count], side, edge bits, unitig, unitig end, degree of an end, palindromic unitig,
 * circular, edge (from, from_rev, to, to_rev), count_sum, n.
 *   interior      U is open and not palindromic, and both its ends have degree >= 1.  Degree is
 *                 kc_clean's: the popcount of the end's edge nibble, self edges included.
 *   neighbours    the multiset N(U) with one entry V for every edge of kc_unitig_graph's list that has
 *                 from = U and to = V != U.  N(U) has at most eight entries.  A V reached by two
 *                 edges counts twice, whether it hangs on both ends of U or twice on one end.  Edges
 *                 that lead back into U -- a hairpin, a homopolymer's loop -- give no entry.
 *                 Neighbours are always open unitigs; they may be palindromic.
 *   local         local_sum = the sum of count_sum(V) and local_n = the sum of n(V) over N(U).
 *   weak          U is weak when N(U) is not empty and either ratio_permille == 0 or
 *                   count_sum(U) * local_n * 1000 < ratio_permille * local_sum * n(U),
 *                 compared strictly and exactly (T(c) is a 32-bit value and ids are below 2^30, so
 *                 each side is below 2^106: the products need 128 bits).  In words: the mean T(c) of
 *                 U is below ratio_permille / 1000 of the mean T(c) over its neighbours' nodes.
 *   cut           U is cut when max_nodes != 0 and n(U) <= max_nodes, the guard passes (max_mean == 0
 *                 or count_sum(U) <= (uint64_t)max_mean * n(U)), and U is interior and weak.
 *   order         every verdict is taken on the one graph, so removals are simultaneous and depend
 *                 on no order.  Cutting joins unitigs, so rounds compose by calling it again on dst,
 *                 and with kc_clean and kc_pop_bubbles by calling one on another's dst.
 *   hazard        the rule knows no parallel arm.  A ratio_permille at or above roughly 500 cuts BOTH
 *                 arms of an even heterozygous bubble: each arm has about half the mean of the two
 *                 unitigs around it.  The customary values are max_nodes = k to 2 k and
 *                 ratio_permille = 100 to 200.
 *   kept nodes    every node of a unitig that is not cut.  Each kept node's raw count (the slot's
 *                 count, not T(c)) is added into dst exactly as kc_table_op_device adds its results:
 *                 a fresh dst holds exactly the cut graph, repeated calls accumulate,
 *                 kc_stats.inserted grows by the counts added, a dst that is too small makes
 *                 kc_finish(dst) return KC_ERR_TABLE_FULL, and a compact snapshot of dst is dropped.
 *                 K-mers of src outside the range are not nodes and are not copied; with max_nodes
 *                 == 0 the call copies the range's nodes.
 *   statistics    dst == NULL fills only the statistics: that call sizes a destination.  nodes ==
 *                 out_keys + cut_nodes always.
 *   kc_cut_weak_device  follows the *_device rule for both contexts as kc_table_op_device does and
 *                 has no host wait; its node ids are sized by src's table slots, as
 *                 kc_unitig_graph_device's.  dev_stats (device memory) may be NULL.
 *   kc_cut_weak   counts the ids first (the k-mers with T(c) >= min_count), runs the ranking once
 *                 and waits for the answer; stats (host memory) may be NULL.
 * Errors: KC_ERR_ARG for dst == src, a different k or device, reserved != 0, min_count above a
 * non-zero max_count, k < 2, a NULL src or desc, ratio_permille > 1000, and max_nodes != 0 with
 * ratio_permille == 0 and max_mean == 0 (that would cut every short interior unitig); KC_ERR_STATE
 * when either context has no table or a failed pass left it incomplete; KC_ERR_NOMEM when the scratch
 * does not fit, reported before any kernel of the call (kc_cut_weak: of the ranking) is launched.  The
 * message goes on dst, or on src when dst is NULL.  An emptied src gives all-zero statistics and adds
 * nothing.  src's table and kc_stats never change.
 * Method: kc_unitigs_device's ranking and its records' kernel as they are, then one pass over the
 * node ids in which the node at position 0 of every open unitig whose ends both have an edge walks
 * the set bits of its two end nibbles, probes each neighbour once, follows slot -> id -> first node,
 * adds that unitig's n and count_sum and writes the verdict at its id; and kc_clean_device's copy of
 * the kept nodes.  An interior unitig costs at most eight probes.  Nothing is added to kc_clean*'s
 * scratch of src:
 *   scratch = 5 * table_slots + 141 * ids bytes,  ids as for kc_unitigs* (< 2^30, else KC_ERR_NOMEM). */
typedef struct {            /* 24 bytes */
    uint32_t min_count, max_count;   /* the range, as kc_graph_device's */
    uint32_t max_nodes;        /* 0: nothing is cut, the call copies the range's nodes */
    uint32_t ratio_permille;   /* 0: no relative test; at most 1000 */
    uint32_t max_mean;         /* 0: no guard */
    uint32_t reserved;         /* 0 */
} kc_weak_desc;
typedef struct {            /* 64 bytes */
    uint64_t unitigs, nodes;   /* of the range's graph: kc_unitig_stats' */
    uint64_t interior;         /* interior unitigs */
    uint64_t weak;             /* interior unitigs that are weak, whatever max_nodes and the guard say */
    uint64_t cut, cut_nodes;   /* cut unitigs and their nodes */
    uint64_t out_keys, out_sum;   /* kept nodes and the sum of their raw counts (added to dst when dst != NULL) */
} kc_weak_stats;
int kc_cut_weak_device(kc_ctx* dst, kc_ctx* src, const kc_weak_desc* d, kc_weak_stats* dev_stats, void* hip_stream);
int kc_cut_weak(kc_ctx* dst, kc_ctx* src, const kc_weak_desc* d, kc_weak_stats* stats);

/* Re-initialise the table, the Bloom filter and all counters (the table/filter
 * constructors again, without reallocating). */
int kc_reset(kc_ctx* ctx);

/* Empty the table only (the next pass that touches it zero-fills it first), keeping the
 * job's counters (windows, chunks, bytes, ...).  The sharded front end calls it on a
 * rank's local table once kc_route_table_device has copied the table out, so the next
 * merge routes only what was counted since (the reference has one shared table and no
 * such step: kmer_hash_table.cpp:2207-2567). */
int kc_clear_table(kc_ctx* ctx);

/* Per-kernel device time, accumulated while profiling is enabled (HIP events on
 * the stream each kernel runs on). */
typedef struct {
    double gather_ms;      /* k_gather (device-image path only) */
    double tokenize_ms;    /* k_tile_summary + k_tile_scan + k_emit */
    double count_ms;       /* k_count (table insert / Bloom pass / gated insert) */
    uint64_t launches;     /* batches timed */
    uint64_t symbols;      /* symbol-stream bytes produced by the timed batches */
} kc_timing;
int kc_profile(kc_ctx* ctx, int enable);
int kc_get_timing(kc_ctx* ctx, kc_timing* t);  /* waits for the timed work; resets the accumulators */

/* Flush staged chunks, wait, and report counters (the timers/counters the functors
 * print, parallel_parser.hpp:1544-1562). stats may be NULL. */
int kc_finish(kc_ctx* ctx, kc_stats* stats);

/* Records {key words[kc_key_words()], T(c)} for every k-mer with T(c) >= a, in
 * table order; key word 0 is most significant, character j of the k-mer is bits
 * 2(k-1-j)..2(k-1-j)+1 of the 64*W-bit integer.  T(c) = c mod 65536 for -m 0,
 * min(c, 16383) otherwise.  Free with kc_free. */
int kc_dump(kc_ctx* ctx, uint64_t** records, uint64_t* n_records);
/* Writes "<CANONICAL_KMER> <T(c)>\n" lines for T(c) >= a (a == 0: nothing written):
 * write_kmers_on_disk_separately_even_faster (kmer_hash_table.cpp:4318-4524) /
 * write_kmers (2013-2050).  Line order is unspecified, as in the reference. */
int kc_write(kc_ctx* ctx, const char* path);
/* Order-independent digest of the text kc_write would write (the reference has none; its
 * output order is unspecified): every line "<CANONICAL_KMER> <T(c)>\n" is
 * hashed with XXH64 (seed 0) over its bytes incl. the '\n'; hash_sum is the sum of those
 * hashes mod 2^64 and hash_xor their XOR.  Any line order gives the same digest, and the digests
 * of disjoint line sets add up (lines, count_sum, hash_sum by addition mod 2^64, hash_xor by XOR),
 * so the owners of a sharded job combine theirs into the whole job's, comparable with a digest of
 * the reference's output file (oracle/kc_digest.c lines).  a == 0: all zero (no output). */
typedef struct {
    uint64_t lines;      /* lines (k-mers with T(c) >= a) */
    uint64_t count_sum;  /* sum of T(c) over the lines */
    uint64_t hash_sum;   /* sum of XXH64(line) mod 2^64 */
    uint64_t hash_xor;   /* XOR of XXH64(line) */
} kc_digest;
int kc_output_digest(kc_ctx* ctx, kc_digest* out);
int kc_key_words(const kc_ctx* ctx);
void kc_free(void* p);

/* Reference chunking of a file image: io_worker (parallel_parser.hpp:1230-1299) +
 * read_chunk_from_file (text_reader.h:93-226) with chunk_size (0 = 10 MiB,
 * main.cpp:387).  *chunks is allocated by the library (kc_free). */
int kc_plan_chunks(const uint8_t* image, uint64_t size, int k, uint64_t chunk_size, int fmt, kc_chunk** chunks,
                   uint64_t* n_chunks);
/* The same chunk table for an image in device memory (after the device's queued work): the
 * planner reads only the bytes around chunk ends, copied to the host in 64 KiB pages on demand,
 * instead of the caller copying the whole image to the host first. */
int kc_plan_chunks_device(const uint8_t* dev_image, uint64_t size, int k, uint64_t chunk_size, int fmt,
                          kc_chunk** chunks, uint64_t* n_chunks);

/* The reference's table size for a minimum of `min_slots` slots: the next prime that is
 * 3 mod 4 (next_prime3mod4, functions_math.cpp:53-96; "Hash table size is:").  The device
 * table keeps 25 % headroom over it (open addressing inside LDS-sized regions), so a job
 * whose distinct k-mers fall between the two succeeds where the reference exits with
 * "Hash table is full"; with KC_STRICT_CAPACITY=1 in the environment (CLI:
 * --strict-capacity) kc_finish returns KC_ERR_TABLE_FULL there too. */
uint64_t kc_table_size_reference(uint64_t min_slots);

/* Test hooks for the Bloom filter (not on the reference's path).
 * kc_xxh64: XXH64(&values[i], 8, seeds[i]) computed by the device function the
 *   reference-layout Bloom passes use (calculate_hashes, double_bloomfilter.hpp:276-281;
 *   xxHash v0.8.2), host arrays in and out.
 * kc_bloom_info: the filter's geometry: words (u32) of its bit array, filter bits per
 *   filter (main.cpp:402-418), ceil(hf) pass-1 and trunc(hf) pass-2 positions
 *   (main.cpp:417, parallel_parser.hpp:2397), layout 1 = blocked (default), 0 = reference.
 * kc_bloom_read / kc_bloom_write: copy the filter's words to / from the host (a write
 *   makes the next pass read the given bits). */
int kc_xxh64(const uint64_t* values, const uint64_t* seeds, uint64_t n, uint64_t* out);
int kc_bloom_info(kc_ctx* ctx, uint64_t* n_words, uint64_t* bits, int* nh, int* nh_gate, int* layout);
int kc_bloom_read(kc_ctx* ctx, uint32_t* words, uint64_t n_words);
int kc_bloom_write(kc_ctx* ctx, const uint32_t* words, uint64_t n_words);

/* Synthetic reads (bench/test input): writes the FASTA records
 * [first_read, first_read + n_reads) of the seeded generator to device memory
 * dev_dst (which receives kc_synth_bytes(first_read, n_reads) bytes). */
uint64_t kc_synth_bytes(uint64_t first_read, uint64_t n_reads, uint32_t read_len, uint32_t wrap);
int kc_synth_device(uint8_t* dev_dst, uint64_t first_read, uint64_t n_reads, uint64_t seed, uint64_t genome_len,
                    uint32_t read_len, uint32_t wrap, double err_rate, double n_rate, void* hip_stream);
/* Skewed variant (bench workloads and skew tests; kc_gen --homo/--dinuc/--repeat):
 * fractions of homopolymer and (CA)n reads, and a repeat of repeat_len bases present
 * repeat_copies times in the genome. */
typedef struct {
    double homo_frac;
    double dinuc_frac;
    uint32_t repeat_len;
    uint32_t repeat_copies;
} kc_synth_skew;
int kc_synth_skew_device(uint8_t* dev_dst, uint64_t first_read, uint64_t n_reads, uint64_t seed, uint64_t genome_len,
                         uint32_t read_len, uint32_t wrap, double err_rate, double n_rate, const kc_synth_skew* skew,
                         void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* KC_API_H */
