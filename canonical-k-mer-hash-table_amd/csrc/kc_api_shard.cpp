// kc_api_shard.cpp -- the entry points of sharded counting (kaarme_amd/sharded.py): routing windows,
// super-k-mers and table records to their owners, inserting received records and keys, and the
// exchange of the sharded Bloom filter (include/kc_api.h).
#include "kc_ctx.h"

extern "C" {

int kc_route_superkmers_device(kc_ctx* c, const uint8_t* img, const kc_chunk* chunks, size_t n, int fmt,
                               uint32_t nshards, int m, uint64_t* dev_pk, uint32_t* dev_bk, uint64_t cap_words,
                               uint64_t* words, uint64_t* windows, void* sp) {
    if (!c || !words || nshards == 0 || nshards > SKM_MAX_SHARDS || (!img && n) || (!chunks && n)) return KC_ERR_ARG;
    if (cap_words && (!dev_pk || !dev_bk)) return KC_ERR_ARG;
    JOB_OK(c);
    const int mm = m ? m : std::min(SKM_DEFAULT_M, c->cfg.k);
    if (mm < 1 || mm > 32 || mm > c->cfg.k) return c->fail(KC_ERR_ARG, "minimizer length must be in 1..min(32, k)");
    hipStream_t s = (hipStream_t)sp;
    const size_t nw = 2 * SKM_MAX_SHARDS + 16;
    if (!c->d_skm.reserve(nw)) return c->fail(KC_ERR_NOMEM, "super-k-mer cursor allocation failed");
    HIPCHK(c, hipMemsetAsync(c->d_skm, 0, nw * 8, s));
    c->skm_shards = nshards;
    c->skm_m = mm;
    c->skm_pk = dev_pk;
    c->skm_bk = dev_bk;
    c->skm_cap = cap_words;
    int rc = device_pass(c, img, chunks, n, fmt, 4, s);
    if (rc) return rc;
    std::vector<unsigned long long> h(nw);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->d_skm, nw * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    uint64_t worst = 0;
    for (uint32_t o = 0; o < nshards; o++) {
        words[o] = h[o];
        if (windows) windows[o] = h[SKM_MAX_SHARDS + o];
        worst = std::max<uint64_t>(worst, h[o]);
    }
    if (cap_words && h[2 * SKM_MAX_SHARDS])
        return c->fail(KC_ERR_NOMEM, "super-k-mer buffer too small: " + std::to_string(worst) +
                                         " words for the largest owner, capacity " + std::to_string(cap_words));
    return KC_OK;
}

int kc_route_device(kc_ctx* c, const uint8_t* img, const kc_chunk* chunks, size_t n, int fmt, uint32_t nshards,
                    uint64_t* dev_out, uint64_t out_capacity, uint64_t* counts, void* sp) {
    if (!c || !counts || !dev_out || nshards == 0 || (!img && n) || (!chunks && n)) return KC_ERR_ARG;
    if (fmt != KC_FMT_FASTA && fmt != KC_FMT_FASTQ && fmt != KC_FMT_PLAIN) return c->fail(KC_ERR_ARG, "unknown format");
    if (c->cfg.bf_enable) return c->fail(KC_ERR_UNSUPPORTED, "sharded counting with the Bloom filter is not supported");
    hipStream_t s = (hipStream_t)sp;
    int rc = flush_host(c);
    if (rc) return rc;
    std::vector<ChunkDesc> batch;
    uint64_t used = 0;
    for (size_t i = 0; i < n; i++) {
        if (!chunks[i].len) continue;
        ChunkDesc d{chunks[i].off, used, chunks[i].len, (uint32_t)(chunks[i].broken_header ? 1 : 0), 0};
        batch.push_back(d);
        used += round_up(chunks[i].len, TILE);
        c->n_chunks++;
        c->n_bytes += chunks[i].len;
    }
    if (used > c->batch_bytes || batch.size() > c->max_chunks)
        return c->fail(KC_ERR_ARG, "kc_route_device: the chunks must fit one staging batch");
    const uint64_t syms = used + batch.size();
    if (out_capacity < syms) return c->fail(KC_ERR_ARG, "kc_route_device: output capacity too small");
    for (uint32_t d = 0; d < nshards; d++) counts[d] = 0;
    if (batch.empty()) return KC_OK;
    StreamScope on(c, s);
    if ((rc = on.join())) return rc;
    rc = ensure_part(c, syms, false, nshards);  // level-1 bins = the shards
    if (rc) return rc;
    if ((uint64_t)nshards * c->pb.nblk1 > c->pb_own.hist1.capacity()) return c->fail(KC_ERR_ARG, "too many shards");
    auto& ev = on.prof.ev;
    if (c->profiling)
        for (int i = 0; i < 4; i++) on.prof.take(i);
    if (c->profiling) HIPCHK(c, hipEventRecord(ev[0], s));
    std::memcpy(c->h_desc[c->cur], batch.data(), batch.size() * sizeof(ChunkDesc));
    HIPCHK(c, hipMemcpyAsync(c->d_chunks, c->h_desc[c->cur], batch.size() * sizeof(ChunkDesc), hipMemcpyHostToDevice, s));
    if (c->profiling) HIPCHK(c, hipEventRecord(ev[1], s));
    const PackedView sv{c->d_pk, c->d_bk};
    HIPCHK(c, launch_tokenize(img, used / TILE, c->d_chunks, (int)batch.size(), fmt, c->d_tiles, c->d_touts,
                              c->d_tblk, sv, syms, c->d_ctr, s));
    if (c->profiling) HIPCHK(c, hipEventRecord(ev[2], s));
    HIPCHK(c, launch_route(sv, c->cfg.k, c->W, c->d_ctr, c->pb, nshards, dev_out, s));
    if ((rc = on.end_profile())) return rc;
    // per-owner totals: off1[d * nblk1], d = 0..nshards (the last one is the total)
    std::vector<uint64_t> offs(nshards + 1);
    for (uint32_t d = 0; d <= nshards; d++)
        HIPCHK(c, hipMemcpyAsync(&offs[d], c->pb.off1 + (uint64_t)d * c->pb.nblk1, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    on.no_hand_back();  // (the call waited for s)
    for (uint32_t d = 0; d < nshards; d++) counts[d] = offs[d + 1] - offs[d];
    return KC_OK;
}

int kc_route_hint(kc_ctx* c, uint32_t nshards) {
    if (!c || nshards > RT_MAX_PARTS) return KC_ERR_ARG;
    int rc = kc_sync(c);  // (the level-3 passes in flight keep the previous pointer)
    if (rc) return rc;
    c->own_parts = nshards;
    return own_prep(c);
}

int kc_route_table_device(kc_ctx* c, uint32_t nshards, uint64_t* dev_out, uint64_t out_capacity, uint64_t* counts,
                          void* sp) {
    if (!c || !counts || nshards == 0 || nshards > 64) return KC_ERR_ARG;
    JOB_OK(c);
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table");
    hipStream_t s = (hipStream_t)sp;
    int rc = flush_host(c);
    if (rc) return rc;
    StreamScope on(c, s);
    if ((rc = on.join())) return rc;
    rc = materialize_zero(c, s);
    if (rc) return rc;
    const uint64_t nblk = (c->nbuckets + 255) / 256, n = nshards * nblk;
    rc = route_bufs(c, n);
    if (rc) return rc;
    if (c->own_parts && !c->pb.own_parts) own_prep(c);  // (d_rhist moved: the level-3 passes follow it)
    const TableView tv = table_view(c);
    if ((rc = on.profile())) return rc;
    // the level-3 passes kept the per-block counts (kc_route_hint): only their scan runs
    const bool kept = c->own_valid && nshards == c->own_parts && c->pb.own_hist == c->d_rhist;
    HIPCHK(c, launch_route_table(tv, nshards, c->d_rhist, c->d_roff, c->d_rbsum, nullptr, s, kept ? 1 : 0));
    c->route_counts_kept += kept;
    c->own_valid = nshards == c->own_parts && c->pb.own_hist == c->d_rhist;  // (the counts of this table)
    std::vector<uint64_t> offs(nshards + 1);
    for (uint32_t d = 0; d <= nshards; d++)
        HIPCHK(c, hipMemcpyAsync(&offs[d], c->d_roff + d * nblk, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    for (uint32_t d = 0; d < nshards; d++) counts[d] = offs[d + 1] - offs[d];
    if (!dev_out) {  // count only (the bracket's events go back to the pool)
        on.no_hand_back();  // (the call waited for s)
        return KC_OK;
    }
    if (out_capacity < offs[nshards])
        return c->fail(KC_ERR_ARG, "kc_route_table_device: output capacity too small (" +
                                       std::to_string(offs[nshards]) + " records)");
    HIPCHK(c, launch_route_table(tv, nshards, c->d_rhist, c->d_roff, c->d_rbsum, dev_out, s));
    if ((rc = on.end_profile())) return rc;
    HIPCHK(c, hipStreamSynchronize(s));
    on.no_hand_back();  // (the call waited for s)
    return KC_OK;
}

}  // extern "C"

// (what the record / key inserts below share: insert_on, kc_ctx.h)

extern "C" {

int kc_insert_counts_device(kc_ctx* c, const uint64_t* recs, uint64_t n, void* sp) {
    if (!c || (!recs && n)) return KC_ERR_ARG;
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table");
    hipStream_t s = (hipStream_t)sp;
    int rc = flush_host(c);
    if (rc) return rc;
    if (n == 0) return KC_OK;
    StreamScope on(c, s);
    const bool part = use_partitioned(c, n);
    return insert_on(
        c, on, false, true,
        [&] {  // records are W + 1 words
            return part ? ensure_part(c, (n * (c->W + 1) + c->W - 1) / c->W, false) : materialize_zero(c, s);
        },
        [&]() -> int {
            HIPCHK(c, launch_insert_counts(recs, n, part, table_view(c), c->d_ctr, c->pb, c->table_fresh, s));
            return KC_OK;
        });
}

int kc_insert_counts_runs_device(kc_ctx* c, const uint64_t* recs, const uint64_t* group_counts, uint32_t ngroups,
                                 void* sp) {
    if (!c || !group_counts || ngroups == 0 || ngroups > 64) return KC_ERR_ARG;
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table");
    std::vector<uint64_t> gs(ngroups + 1, 0);
    uint64_t maxn = 0;
    for (uint32_t g = 0; g < ngroups; g++) {
        gs[g + 1] = gs[g] + group_counts[g];
        maxn = std::max(maxn, group_counts[g]);
    }
    const uint64_t n = gs[ngroups];
    if (!recs && n) return KC_ERR_ARG;
    hipStream_t s = (hipStream_t)sp;
    int rc = flush_host(c);
    if (rc) return rc;
    if (n == 0) return KC_OK;
    StreamScope on(c, s);
    if ((rc = on.join())) return rc;
    const uint64_t need = (c->R + 1) * ngroups;
    if (!c->d_gstart.reserve(65)) return c->fail(KC_ERR_NOMEM, "merge buffer allocation failed");
    if (!reserve_pair(c->d_mstart, need, c->d_mlen, need))
        return c->fail(KC_ERR_NOMEM, "merge buffer allocation failed");
    HIPCHK(c, hipMemcpyAsync(c->d_gstart, gs.data(), (ngroups + 1) * 8, hipMemcpyHostToDevice, s));
    // the groups must be sorted by this table's region (a sender table of another geometry,
    // or records not from kc_route_table_device, take the general merge insert)
    unsigned long long* flag = &c->d_ctr->part_overflow;
    HIPCHK(c, hipMemsetAsync(flag, 0, 8, s));
    TableView tv = table_view(c);
    HIPCHK(c, launch_check_runs(recs, c->d_gstart, ngroups, maxn, tv, flag, s));
    unsigned long long unsorted = 0;
    HIPCHK(c, hipMemcpyAsync(&unsorted, flag, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (unsorted) {
        on.no_hand_back();  // (the call waited for s; the general insert joins and hands back itself)
        return kc_insert_counts_device(c, recs, n, sp);
    }
    // records counted like kc_insert_counts_device: inserted += their counts
    return insert_on(
        c, on, false, false, [] { return (int)KC_OK; },
        [&]() -> int {
            HIPCHK(c, launch_insert_counts_runs(recs, c->d_gstart, ngroups, tv, c->d_ctr, c->d_mlen, c->d_mstart,
                                                c->table_fresh, s));
            return KC_OK;
        });
}

int kc_bloom_records_device(kc_ctx* c, const uint64_t* recs, uint64_t n, void* sp) {
    if (!c || (!recs && n)) return KC_ERR_ARG;
    if (!c->cfg.bf_enable || c->bloom_final) return c->fail(KC_ERR_STATE, "bloom pass not active");
    if (!c->bloom_blocked) return c->fail(KC_ERR_ARG, "records need the blocked Bloom layout");
    hipStream_t s = (hipStream_t)sp;
    int rc = flush_host(c);
    if (rc) return rc;
    c->bloom_batches++;  // (a Bloom pass of records keeps no partitions)
    c->reuse_kept = false;
    if (n == 0) return KC_OK;
    StreamScope on(c, s);
    // exact-layout levels for items of W + 1 words in the filter's region geometry
    const PartGeo g{c->bgeo.F1, c->bgeo.F2, c->bgeo.R, c->W + 1};
    const BloomView bv{c->d_bloom, c->bf_bits ? c->bf_bits - 1 : 0, c->nh, c->nh_gate, c->bloom_blocked,
                       bloom_blocks(c->bf_bits)};
    return insert_on(
        c, on, true, false, [&] { return ensure_part_geo(c, n, false, g, c->pbf, c->pbf_own); },
        [&]() -> int {
            HIPCHK(c, launch_bloom_records(c->W, recs, n, bv, c->bgeo, c->d_ctr, c->pbf, c->bloom_fresh, s));
            return KC_OK;
        });
}

int kc_count_records_device(kc_ctx* c, const uint64_t* recs, uint64_t n, void* sp) {
    if (!c || (!recs && n)) return KC_ERR_ARG;
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table (kc_bloom_finalize must precede the counting pass)");
    const bool gate = c->cfg.bf_enable && c->cfg.mode != 1;  // -m 1 -b ignores the filter (main.cpp:482-489)
    if (gate && !c->bloom_blocked) return c->fail(KC_ERR_ARG, "records need the blocked Bloom layout");
    hipStream_t s = (hipStream_t)sp;
    int rc = flush_host(c);
    if (rc) return rc;
    if (n == 0) return KC_OK;
    StreamScope on(c, s);
    const BloomView bv{c->d_bloom, c->bf_bits ? c->bf_bits - 1 : 0, c->nh, c->nh_gate, c->bloom_blocked,
                       bloom_blocks(c->bf_bits)};
    return insert_on(
        c, on, false, false,
        [&] { return ensure_part(c, (n * (c->W + 1) + c->W - 1) / c->W, false); },  // records: W + 1 words
        [&]() -> int {
            HIPCHK(c, launch_count_records(c->W, recs, n, table_view(c), bv, c->d_ctr, c->pb, c->table_fresh,
                                           gate ? 1 : 0, s));
            return KC_OK;
        });
}

int kc_insert_keys_device(kc_ctx* c, const uint64_t* keys, uint64_t n, void* sp) {
    if (!c || (!keys && n)) return KC_ERR_ARG;
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table");
    hipStream_t s = (hipStream_t)sp;
    int rc = flush_host(c);
    if (rc) return rc;
    if (n == 0) return KC_OK;
    StreamScope on(c, s);
    const bool part = use_partitioned(c, n);
    // (the bracket opens after the levels are sized, before a direct insert's deferred reset)
    return insert_on(
        c, on, false, false, [&] { return part ? ensure_part(c, n, false) : (int)KC_OK; },
        [&]() -> int {
            if (!part) {
                const int rz = materialize_zero(c, s);
                if (rz) return rz;
            }
            HIPCHK(c, launch_insert_keys(keys, n, part, table_view(c), c->d_ctr, c->pb, c->table_fresh, s));
            return KC_OK;
        });
}

// Work on the scope's stream after everything the context staged from the host (its own stream).
// Their success paths end with no_hand_back(): kc_bloom_set_device and kc_bloom_estimate wait for s,
// and kc_bloom_get_device only reads the filter (its copy has never been handed back).
static int after_host_work(kc_ctx* c, StreamScope& on) {
    int rc = flush_host(c);
    if (rc) return rc;
    return on.join();
}

int kc_bloom_get_device(kc_ctx* c, uint32_t* dev_dst, uint64_t first_word, uint64_t n_words, void* sp) {
    if (!c || (!dev_dst && n_words)) return KC_ERR_ARG;
    if (!c->d_bloom) return c->fail(KC_ERR_STATE, "no Bloom filter");
    if (first_word > bloom_words(c) || n_words > bloom_words(c) - first_word)
        return c->fail(KC_ERR_ARG, "word range outside the filter");
    hipStream_t s = (hipStream_t)sp;
    StreamScope on(c, s);
    int rc = after_host_work(c, on);
    if (rc) return rc;
    if (n_words) HIPCHK(c, hipMemcpyAsync(dev_dst, c->d_bloom + first_word, n_words * 4, hipMemcpyDeviceToDevice, s));
    on.no_hand_back();
    return KC_OK;
}

int kc_bloom_merge_device(kc_ctx* c, const uint32_t* dev_parts, uint32_t nparts, uint64_t n_words, uint32_t* dev_out,
                          void* sp) {
    if (!c || nparts == 0 || (n_words && (!dev_parts || !dev_out))) return KC_ERR_ARG;
    if (!c->d_bloom) return c->fail(KC_ERR_STATE, "no Bloom filter");
    if (c->bloom_blocked && n_words % 16) return c->fail(KC_ERR_ARG, "the blocked filter merges whole 16-word blocks");
    HIPCHK(c, launch_bloom_merge(dev_parts, nparts, n_words, c->bloom_blocked, dev_out, (hipStream_t)sp));
    return KC_OK;
}

// Distinct k-mers in filter 2 from its set bits (after the work queued on s): X of m bits set
// after n insertions of h positions each, X = m (1 - e^{-hn/m}).
static int estimate_filter2(kc_ctx* c, hipStream_t s, uint64_t* est) {
    unsigned long long* part_d = c->d_sum + CHECKSUM_SLOTS;  // the first CHECKSUM_SLOTS hold the reuse checksum
    HIPCHK(c, launch_bloom_popcount2(c->d_bloom, bloom_words(c), c->bloom_blocked, part_d, s));
    unsigned long long part[CHECKSUM_SLOTS];
    HIPCHK(c, hipMemcpyAsync(part, part_d, sizeof(part), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    double x = 0;
    for (auto v : part) x += (double)v;
    const double m = c->bloom_blocked ? 256.0 * (double)bloom_blocks(c->bf_bits) : (double)c->bf_bits;
    x = std::min(x, m - 1);
    *est = (uint64_t)std::llround(-(m / std::max(1, c->nh)) * std::log1p(-x / m));
    return KC_OK;
}

int kc_bloom_set_device(kc_ctx* c, const uint32_t* dev_src, uint64_t n_words, uint64_t* new_in_second, void* sp) {
    if (!c || !dev_src) return KC_ERR_ARG;
    if (!c->cfg.bf_enable || c->bloom_final) return c->fail(KC_ERR_STATE, "bloom pass not active");
    if (n_words != bloom_words(c)) return c->fail(KC_ERR_ARG, "n_words must be the filter's word count");
    hipStream_t s = (hipStream_t)sp;
    StreamScope on(c, s);
    int rc = after_host_work(c, on);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(c->d_bloom, dev_src, n_words * 4, hipMemcpyDeviceToDevice, s));
    c->bloom_fresh = false;
    uint64_t est = 0;
    rc = estimate_filter2(c, s, &est);  // waits for the copy
    if (rc) return rc;
    // the pass-1 counter kc_bloom_finalize sizes the table from (main.cpp:454)
    HIPCHK(c, hipMemcpy(&c->d_ctr->new_in_second, &est, 8, hipMemcpyHostToDevice));
    if (new_in_second) *new_in_second = est;
    on.no_hand_back();  // (estimate_filter2 waited for s)
    return KC_OK;
}

int kc_bloom_estimate(kc_ctx* c, uint64_t* distinct_in_second, void* sp) {
    if (!c || !distinct_in_second) return KC_ERR_ARG;
    if (!c->d_bloom) return c->fail(KC_ERR_STATE, "no Bloom filter");
    hipStream_t s = (hipStream_t)sp;
    StreamScope on(c, s);
    int rc = after_host_work(c, on);
    if (rc) return rc;
    if ((rc = estimate_filter2(c, s, distinct_in_second))) return rc;
    on.no_hand_back();  // (estimate_filter2 waited for s)
    return KC_OK;
}

}  // extern "C"
