// kc_api_pass.cpp -- the passes over input: one batch through the tokenizer and the insert path
// chosen for it (run_batch), the deferred level 3, the pass over a device image (device_pass), the
// counting pass from the Bloom pass's kept partitions (count_reused), the staging of host chunks,
// and the count / bloom / estimate / finalize entry points (include/kc_api.h).
#include "kc_ctx.h"

// ------------------------------------------------------------------------------
// batch execution
// ------------------------------------------------------------------------------
// src: the bytes the chunk descriptors' src_off point into (the host stage, or a
// device-resident image read in place)
// The tail of a segmented batch (the skew list, the batch's bookkeeping, the exact pipeline
// behind the device overflow gate) does nothing unless the single-pass levels left a skew list
// or overflowed.  For device images the host reads those two counters after the main phase
// (the call waits for its batch) and launches the tail only when needed: ~20 idle kernel
// launches and two region-grid passes less per batch (0.25 ms of C2's 15.9 ms step).  Images
// of several batches and host chunks keep the device gate (their batches queue behind each
// other).
static int tail_needed(kc_ctx* c, hipStream_t s, bool* need) {
    unsigned long long f[2] = {0, 0};
    HIPCHK(c, hipMemcpyAsync(&f[0], &c->d_ctr->part_overflow, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&f[1], &c->d_ctr->spill_n, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    *need = f[0] != 0 || f[1] != 0;
    return KC_OK;
}

// a device counter set from the host, in stream order
static hipError_t set_dev_u64(unsigned long long* p, uint64_t v, hipStream_t s) {
    hipError_t e = hipMemsetD32Async((hipDeviceptr_t)p, (int)(uint32_t)v, 1, s);
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)((uint32_t*)p + 1), (int)(uint32_t)(v >> 32), 1, s);
    return e;
}

// The level-3 pass of the deferred group (run_deferred): the waiting batches' segments, slots of
// batches that did not fill the group zeroed first (their fills are a previous group's)
static int flush_deferred(kc_ctx* c, const PackedView& sv, uint64_t syms, int mode, const TableView& tv,
                          const BloomView& bv, PartBufs pb, hipStream_t s, bool overflowed) {
    const uint32_t G = c->defer_g, B2 = c->pb.B2;
    // (the batch that overflowed: its segments are not all written; its tail redoes it)
    const uint32_t keep = overflowed ? c->defer_n - 1 : c->defer_n;
    if (keep < G)
        HIPCHK(c, hipMemset2DAsync(c->pb.hist2 + (uint64_t)keep * B2, (size_t)G * B2 * 4, 0, (size_t)(G - keep) * B2 * 4,
                                   c->R, s));
    if (overflowed) HIPCHK(c, launch_hold_overflow(c->d_ctr, 0, s));
    HIPCHK(c, launch_count_partitioned(sv, syms, c->cfg.k, mode, tv, bv, c->d_ctr, pb, c->table_fresh, s, PH_L3));
    if (overflowed) HIPCHK(c, launch_hold_overflow(c->d_ctr, 1, s));
    c->table_zero_pending = false;  // a fresh level 3 writes every region
    own_after_write(c, true, c->table_fresh);
    c->table_fresh = false;
    c->defer_n = 0;
    c->defer_groups++;
    return KC_OK;
}

// One batch of a deferred counting pass: levels 1-2 into the batch's slot of the group's level-2
// segments; the group's level 3 when the group is full, at the pass's last batch, or when this
// batch needs its tail (a skew list, or segments that overflowed: the tail's exact pipeline uses
// the key buffers as scratch, so the waiting segments are inserted first).  The host reads the
// batch's two flags (it waits for the batch) before queueing the next one.
static int run_deferred(kc_ctx* c, const PackedView& sv, uint64_t syms, int mode, const TableView& tv,
                        const BloomView& bv, hipStream_t s) {
    PartBufs pb = c->pb;
    pb.b2t = c->defer_g * pb.B2;
    pb.b2off = c->defer_n * pb.B2;
    pb.keep_skew = c->defer_n > 0;  // (the group's skew list so far stays)
    HIPCHK(c, launch_count_partitioned(sv, syms, c->cfg.k, mode, tv, bv, c->d_ctr, pb, c->table_fresh, s, PH_L12));
    c->defer_n++;
    unsigned long long f[3] = {0, 0, 0};
    HIPCHK(c, hipMemcpyAsync(&f[0], &c->d_ctr->part_overflow, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&f[1], &c->d_ctr->spill_n, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&f[2], &c->d_ctr->heavy_n, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const bool overflowed = f[0] != 0;
    // a skew list alone does not end the group: the next batch appends to it
    if (!overflowed && c->defer_n < c->defer_g && !c->defer_last) {
        c->skew_prev = f[1];
        c->heavy_prev = f[2];
        return KC_OK;
    }
    int rc = flush_deferred(c, sv, syms, mode, tv, bv, pb, s, overflowed);
    if (rc) return rc;
    if (overflowed && c->skew_prev) {
        // this batch is redone by the exact pipeline (its tail); the list's first skew_prev entries
        // are the group's earlier batches' and are inserted first, with the overflow flag held
        HIPCHK(c, launch_hold_overflow(c->d_ctr, 0, s));
        HIPCHK(c, set_dev_u64(&c->d_ctr->spill_n, c->skew_prev, s));
        HIPCHK(c, set_dev_u64(&c->d_ctr->heavy_n, c->heavy_prev, s));
        HIPCHK(c, launch_count_partitioned(sv, syms, c->cfg.k, mode, tv, bv, c->d_ctr, c->pb, c->table_fresh, s,
                                           PH_TAIL));
        HIPCHK(c, set_dev_u64(&c->d_ctr->spill_n, 0, s));
        HIPCHK(c, set_dev_u64(&c->d_ctr->heavy_n, 0, s));
        HIPCHK(c, launch_hold_overflow(c->d_ctr, 1, s));
    }
    c->skew_prev = c->heavy_prev = 0;
    if (overflowed || f[1] != 0)
        HIPCHK(c, launch_count_partitioned(sv, syms, c->cfg.k, mode, tv, bv, c->d_ctr, c->pb, c->table_fresh, s,
                                           PH_TAIL));
    return KC_OK;
}

// pre: a symbol stream already in HBM (a received super-k-mer stream, kc_count_packed_device) of
// `used` symbols instead of chunks to tokenize (src, nchunks and fmt unused); pre_len: the device
// word holding its actual length when `used` only bounds it (a batch the estimate pass tokenized)
static int run_batch(kc_ctx* c, const uint8_t* src, uint64_t used, uint64_t nchunks, int fmt, int pass, hipStream_t s,
                     ProfEvents* started = nullptr, bool keep = false,
                     bool host_gate = false, const PackedView* pre = nullptr, const uint64_t* pre_len = nullptr) {
    ProfEvents own(c);  // (or the quadruple the caller started: device_pass)
    ProfEvents& prof = started ? *started : own;
    auto& ev = prof.ev;
    const uint64_t ntiles = used / TILE;
    if (!pre && ntiles == 0) return KC_OK;
    if (pre && used == 0) return KC_OK;
    if (pass == 3) {  // the distinct-count sketch (kc_estimate_distinct_device): tokenize + k_hll
        PackedView v{c->d_pk, c->d_bk};
        const uint64_t words = (used + nchunks) / 32 + 4;
        const bool kept = c->keep_target && c->keep_woff + words <= c->keep_pk.capacity() &&
                          c->kept.size() < c->d_kept_len.capacity();
        if (kept) {  // (kept for the counting pass)
            v = PackedView{c->keep_pk + c->keep_woff, c->keep_bk + c->keep_woff};
            c->kept.emplace_back(c->keep_woff, used + nchunks);
            c->keep_woff += words;
        } else {
            c->keep_target = false;
        }
        HIPCHK(c, launch_tokenize(src, ntiles, c->d_chunks, (int)nchunks, fmt, c->d_tiles, c->d_touts, c->d_tblk, v,
                                  used + nchunks, c->d_ctr, s));
        if (kept)  // the batch's stream length (the tokenizer's, below the bound)
            HIPCHK(c, hipMemcpyAsync(c->d_kept_len + c->kept.size() - 1, &c->d_ctr->stream_len, 8,
                                     hipMemcpyDeviceToDevice, s));
        HIPCHK(c, launch_hll(v, c->cfg.k, c->W, c->d_ctr, c->d_hll, s));
        if (kept)  // the windows so far (the batch's: the difference to the previous batch's)
            HIPCHK(c, hipMemcpyAsync(c->d_kept_win + c->kept.size() - 1, &c->d_ctr->est_windows, 8,
                                     hipMemcpyDeviceToDevice, s));
        return KC_OK;
    }
    if (pass == 4) {  // super-k-mer routing (kc_route_superkmers_device): tokenize + k_skm_route
        const PackedView v{c->d_pk, c->d_bk};
        HIPCHK(c, launch_tokenize(src, ntiles, c->d_chunks, (int)nchunks, fmt, c->d_tiles, c->d_touts, c->d_tblk, v,
                                  used + nchunks, c->d_ctr, s));
        HIPCHK(c, launch_skm_route(v, c->d_ctr, used + nchunks, c->cfg.k, c->skm_m, c->skm_shards, c->skm_pk,
                                   c->skm_bk, c->skm_cap, c->d_skm, c->d_skm + SKM_MAX_SHARDS,
                                   c->d_skm + 2 * SKM_MAX_SHARDS, s));
        return KC_OK;
    }
    if (c->profiling) {
        if (!ev[0]) {
            prof.take(0);
            prof.take(1);
            HIPCHK(c, hipEventRecord(ev[0], s));
            HIPCHK(c, hipEventRecord(ev[1], s));
        }
        prof.take(2);
        prof.take(3);
    }
    const PackedView sv = pre ? *pre : PackedView{c->d_pk, c->d_bk};
    if (pre) {  // (the stream's length where the tokenizer would have left it)
        if (pre_len) {
            HIPCHK(c, hipMemcpyAsync(&c->d_ctr->stream_len, pre_len, 8, hipMemcpyDeviceToDevice, s));
        } else {
            HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)&c->d_ctr->stream_len, (int)(uint32_t)used, 1, s));
            HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)((uint32_t*)&c->d_ctr->stream_len + 1),
                                        (int)(uint32_t)(used >> 32), 1, s));
        }
        nchunks = 0;
    } else {
        HIPCHK(c, launch_tokenize(src, ntiles, c->d_chunks, (int)nchunks, fmt, c->d_tiles, c->d_touts, c->d_tblk, sv,
                                  used + nchunks, c->d_ctr, s));
    }
    if (c->profiling) HIPCHK(c, hipEventRecord(ev[2], s));
    TableView tv = table_view(c);
    BloomView bv{c->d_bloom, c->bf_bits ? c->bf_bits - 1 : 0, c->nh, c->nh_gate, c->bloom_blocked,
                 bloom_blocks(c->bf_bits)};
    int mode;
    if (pass == 1) mode = 1;
    else mode = (c->cfg.bf_enable && c->cfg.mode != 1) ? 2 : 0;  // -m 1 -b ignores the filter (main.cpp:482-489)
    const uint64_t syms = used + nchunks;
    if (mode == 1) {
        c->bloom_batches++;
        c->reuse_kept = false;
    }
    if (mode == 1 && c->bloom_blocked && use_partitioned_bloom(c, syms)) {
        const bool seg = insert_path_knob() != PathKnob::Exact;
        keep = keep && seg;  // (the exact layout does not keep: its level 1 moves word 0 only)
        keep = keep && c->fgeo.R != 0;
        const PartGeo g = keep ? PartGeo{c->fgeo.F1, c->fgeo.F2, c->fgeo.R, c->W}
                               : PartGeo{c->bgeo.F1, c->bgeo.F2, c->bgeo.R, 1};
        int rc = ensure_part_geo(c, syms, seg, g, c->pbf, c->pbf_own);
        if (rc) return rc;
        c->pbf.keep_fill = c->pbf.keep_fill2 = nullptr;
        if (keep) {  // copies of the kept partitions' segment fills
            if (!c->d_keep_fill.reserve((uint64_t)c->fgeo.F1 * c->pbf.nblk1) ||
                !c->d_keep_fill2.reserve(c->fgeo.R * c->pbf.B2))
                return c->fail(KC_ERR_NOMEM, "partition fill copy allocation failed");
            c->pbf.keep_fill = c->d_keep_fill.get();
            c->pbf.keep_fill2 = c->d_keep_fill2.get();
        }
        // two-word keys: the kept levels as 12-byte records (kc_count_impl.h Rec12) when a record
        // holds the table key's bits below its bin: hb + 1 + xb <= 32 at both levels
        c->pbf.rec12 = 0;
        if (keep && c->W == 2) {
            int f1 = 0, rb = 0;
            while ((1u << f1) < c->fgeo.F1) f1++;
            while ((1ULL << rb) < c->fgeo.R) rb++;
            const int hb = std::max(0, 2 * c->cfg.k - 96);
            int b2s = 0;
            while ((1u << b2s) < c->pbf.B2) b2s++;
            if (hb + 1 + (32 - f1) <= 32 && hb + 1 + (32 - rb) <= 32 && f1 >= 1 && (1u << b2s) == c->pbf.B2) {
                c->pbf.rec12 = R12_P1 | R12_IN | R12_OUT | R12_L2;
                c->pbf.r12_hb = hb;
                c->pbf.r12_xb1 = 32 - f1;
                c->pbf.r12_xb2 = 32 - rb;
                c->pbf.r12_b2s = b2s;
            }
        }
        const bool split = host_gate && c->pbf.cap1 != 0;
        bool tail = false;
        HIPCHK(c, launch_bloom_partitioned(sv, c->cfg.k, c->W, bv, c->bgeo, c->fgeo, c->d_ctr, c->pbf, c->bloom_fresh,
                                           keep ? 1 : 0, s, split ? PH_MAIN : PH_ALL));
        if (split && (rc = tail_needed(c, s, &tail))) return rc;
        if (tail)
            HIPCHK(c, launch_bloom_partitioned(sv, c->cfg.k, c->W, bv, c->bgeo, c->fgeo, c->d_ctr, c->pbf,
                                               c->bloom_fresh, keep ? 1 : 0, s, PH_TAIL));
        c->bloom_fresh = false;
        c->reuse_kept = keep;
    } else if (mode != 1 && c->defer_on) {  // (device_pass chose the partitioned segmented path)
        int rc = ensure_part(c, std::max(syms, c->defer_syms), true, 0, c->defer_g);
        if (rc) return rc;
        if (c->pb.cap1 == 0) return c->fail(KC_ERR_STATE, "deferred level 3 without segmented levels");
        if ((rc = run_deferred(c, sv, syms, mode, tv, bv, s))) return rc;
    } else if (mode != 1 && use_partitioned(c, syms)) {
        int rc = ensure_part(c, syms, insert_path_knob() != PathKnob::Exact);
        if (rc) return rc;
        const bool split = host_gate && c->pb.cap1 != 0;
        HIPCHK(c, launch_count_partitioned(sv, syms, c->cfg.k, mode, tv, bv, c->d_ctr, c->pb, c->table_fresh, s,
                                           split ? PH_MAIN : PH_ALL));
        bool tail = false;
        if (split && (rc = tail_needed(c, s, &tail))) return rc;
        if (tail)
            HIPCHK(c, launch_count_partitioned(sv, syms, c->cfg.k, mode, tv, bv, c->d_ctr, c->pb, c->table_fresh, s,
                                               PH_TAIL));
        c->table_zero_pending = false;  // the fresh pass wrote every region
        own_after_write(c, true, c->table_fresh);
    } else {
        if (mode != 1) {
            const int rc = materialize_zero(c, s);
            if (rc) return rc;
            own_after_write(c, false, false);
        }
        HIPCHK(c, launch_count(sv, syms, c->cfg.k, mode, tv, bv, c->d_ctr, s));
        if (mode == 1) c->bloom_fresh = false;
    }
    if (mode != 1 && !c->defer_on) c->table_fresh = false;  // (a deferred pass: its level 3 clears it)
    if (c->profiling) {
        HIPCHK(c, hipEventRecord(ev[3], s));
        prof.commit();
    }
    return KC_OK;
}

int flush_host(kc_ctx* c) {
    if (c->cur_n == 0) return KC_OK;
    const int b = c->cur;
    HIPCHK(c, hipMemcpyAsync(c->d_stage, c->h_stage[b], c->cur_used, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_chunks, c->h_desc[b], c->cur_n * sizeof(ChunkDesc), hipMemcpyHostToDevice,
                             c->stream));
    HIPCHK(c, hipEventRecord(c->h_free[b], c->stream));
    int rc = run_batch(c, c->d_stage, c->cur_used, c->cur_n, c->cur_fmt, c->cur_pass, c->stream);
    if (rc) return rc;
    c->cur ^= 1;
    c->cur_used = 0;
    c->cur_n = 0;
    HIPCHK(c, hipEventSynchronize(c->h_free[c->cur]));  // buffer we fill next is no longer read
    return KC_OK;
}

static int add_host_chunk(kc_ctx* c, const uint8_t* buf, size_t len, int fmt, int bh, int pass) {
    if (!buf && len) return c->fail(KC_ERR_ARG, "null buffer");
    if (fmt != KC_FMT_FASTA && fmt != KC_FMT_FASTQ && fmt != KC_FMT_PLAIN) return c->fail(KC_ERR_ARG, "unknown format");
    if (len == 0) return KC_OK;
    const uint64_t need = round_up(len, TILE);
    if (need > c->batch_bytes) return c->fail(KC_ERR_ARG, "chunk larger than the staging batch");
    if (c->cur_n && (c->cur_fmt != fmt || c->cur_pass != pass || c->cur_used + need > c->batch_bytes ||
                     c->cur_n + 1 > c->max_chunks)) {
        int rc = flush_host(c);
        if (rc) return rc;
    }
    ChunkDesc d;
    d.src_off = c->cur_used;  // host chunks are tokenized from the stage itself
    d.stage_off = c->cur_used;
    d.len = len;
    d.bh = bh ? 1 : 0;
    d.pad = 0;
    if (!c->h_stage[c->cur]) {  // host chunks: two pinned stages + the device stage, on first use
        for (int i = 0; i < 2; i++)
            if (!c->h_stage[i].reserve(c->batch_bytes))
                return c->fail(KC_ERR_NOMEM, "pinned staging allocation failed");
        if (!c->d_stage.reserve(c->batch_bytes))
            return c->fail(KC_ERR_NOMEM, "device stage allocation failed");
    }
    std::memcpy(c->h_stage[c->cur] + c->cur_used, buf, len);
    c->h_desc[c->cur][c->cur_n++] = d;
    c->cur_used += need;
    c->cur_fmt = fmt;
    c->cur_pass = pass;
    if (pass == 0) { c->n_chunks++; c->n_bytes += len; }
    return KC_OK;
}

static bool reuse_enabled() {
    const char* v = std::getenv("KC_REUSE");
    return !(v && *v == '0');
}

// The counting pass from the Bloom pass's kept level-1 output (see kc_ctx, level-1 reuse).
// Sets *done when the pass ran; otherwise (different input, changed bytes, overflow) the
// caller runs the ordinary pass and nothing was counted.
static int count_reused(kc_ctx* c, const uint8_t* img, const kc_chunk* chunks, size_t n, int fmt, hipStream_t s,
                        bool* done) {
    *done = false;
    if (img != c->reuse_img || fmt != c->reuse_fmt) {
        if (debug_on()) std::fprintf(stderr, "reuse: another image or format\n");
        return KC_OK;
    }
    std::vector<ChunkDesc> b;
    uint64_t used = 0, max_len = 0, bytes = 0;
    for (size_t i = 0; i < n; i++) {
        if (chunks[i].len == 0) continue;
        ChunkDesc d;
        d.src_off = chunks[i].off;
        d.stage_off = used;
        d.len = chunks[i].len;
        d.bh = chunks[i].broken_header ? 1 : 0;
        d.pad = 0;
        b.push_back(d);
        used += round_up(chunks[i].len, TILE);
        max_len = std::max<uint64_t>(max_len, d.len);
        bytes += d.len;
    }
    if (b.size() != c->reuse_chunks.size() || used != c->reuse_used) return KC_OK;
    for (size_t i = 0; i < b.size(); i++) {
        const ChunkDesc &x = b[i], &y = c->reuse_chunks[i];
        if (x.src_off != y.src_off || x.len != y.len || x.bh != y.bh) return KC_OK;
    }
    int rc = flush_host(c);  // keep order with staged host chunks
    if (rc) return rc;
    StreamScope on(c, s);
    if ((rc = on.join())) return rc;
    auto& ev = on.prof.ev;
    if (c->profiling)
        for (int i = 0; i < 4; i++) on.prof.take(i);
    if (ev[0]) {
        HIPCHK(c, hipEventRecord(ev[0], s));
        HIPCHK(c, hipEventRecord(ev[1], s));
    }
    // the bytes must be the Bloom pass's: same checksum.  It runs on the aux stream beside the
    // counting pass from the partitions (which reads no input byte); a mismatch restores the
    // counters and drops the table before the ordinary pass (C3: 0.35 ms off the step)
    std::memcpy(c->h_desc[c->cur], b.data(), b.size() * sizeof(ChunkDesc));
    HIPCHK(c, hipMemcpyAsync(c->d_chunks, c->h_desc[c->cur], b.size() * sizeof(ChunkDesc), hipMemcpyHostToDevice, s));
    if (!c->aux) {
        HIPCHK(c, hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
        for (auto& e : c->aev) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    HIPCHK(c, hipEventRecord(c->aev[0], s));
    HIPCHK(c, hipStreamWaitEvent(c->aux, c->aev[0], 0));
    HIPCHK(c, launch_checksum(img, c->d_chunks, (int)b.size(), max_len, c->d_sum, c->aux));
    HIPCHK(c, hipMemcpyAsync(c->h_part, c->d_sum, sizeof(c->h_part), hipMemcpyDeviceToHost, c->aux));
    HIPCHK(c, hipEventRecord(c->aev[1], c->aux));
    auto same_bytes = [&](bool* same) -> int {  // waits for the checksum
        HIPCHK(c, hipEventSynchronize(c->aev[1]));
        unsigned long long sum = 0;
        for (auto v : c->h_part) sum += v;
        *same = sum == c->reuse_sum;
        if (!*same && debug_on()) std::fprintf(stderr, "reuse: checksum differs\n");
        return KC_OK;
    };
    if (ev[2]) HIPCHK(c, hipEventRecord(ev[2], s));
    bool same = false;
    const uint64_t syms = used + b.size();
    // the table's partition buffers for this batch, with the Bloom pass's partitions as its
    // level 1 (and level 2); the kept buffers must not have moved
    if ((rc = ensure_part(c, syms, true))) return rc;
    PartBufs pr = c->pb;
    if (pr.keys1 != c->pbf.keys1 || (c->reuse_level == 2 && pr.keys2 != c->pbf.keys2) || pr.nblk1 != c->pbf.nblk1 ||
        pr.B2 != c->pbf.B2 || pr.cap1 != c->pbf.cap1 || pr.cap1 == 0 || c->F1 != c->fgeo.F1) {
        if (debug_on()) std::fprintf(stderr, "reuse: partition geometry differs\n");
        HIPCHK(c, hipEventSynchronize(c->aev[1]));
        on.no_hand_back();  // (nothing was counted; the ordinary pass joins again)
        return KC_OK;
    }
    pr.hist1 = c->d_keep_fill;
    // the kept records' format: level 2 read by level 3, or level 1 read by level 2 (which then
    // writes whole keys in the table's own geometry)
    pr.rec12 = c->pbf.rec12 ? (c->reuse_level == 2 ? R12_L2 : R12_IN) : 0;
    pr.r12_hb = c->pbf.r12_hb;
    pr.r12_xb1 = c->pbf.r12_xb1;
    pr.r12_xb2 = c->pbf.r12_xb2;
    pr.r12_b2s = c->pbf.r12_b2s;
    if (c->reuse_level == 2) {  // a table region = fgeo.R / R consecutive fine bins
        pr.hist2 = c->d_keep_fill2;
        pr.cap2 = c->pbf.cap2;
        pr.B2 = (uint32_t)(c->fgeo.R / c->R) * c->pbf.B2;
    }
    const BloomView bv{c->d_bloom, c->bf_bits ? c->bf_bits - 1 : 0, c->nh, c->nh_gate, c->bloom_blocked,
                       bloom_blocks(c->bf_bits)};
    // the counters as they were, for a redo (other bytes, or a table region that overflowed)
    DevCounters before;
    HIPCHK(c, hipMemcpyAsync(&before, c->d_ctr, sizeof(before), hipMemcpyDeviceToHost, s));
    // -m 1 -b counts every window (the reference ignores its filter, main.cpp:482-489)
    HIPCHK(c, launch_count_reuse(c->W, table_view(c), bv, c->d_ctr, pr, c->table_fresh, c->reuse_level,
                                 c->cfg.mode != 1, c->reuse_windows, s));
    if (ev[3]) HIPCHK(c, hipEventRecord(ev[3], s));
    unsigned long long ovf = 0, full = 0;
    HIPCHK(c, hipMemcpyAsync(&ovf, &c->d_ctr->part_overflow, sizeof(ovf), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipMemcpyAsync(&full, &c->d_ctr->overflow, sizeof(full), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if ((rc = same_bytes(&same))) return rc;
    if (!same || ovf || full != before.overflow) {
        // other bytes than the Bloom pass's, a full skew list, or a region of the table sized for
        // the gated k-mers that overflowed: the ordinary counting pass redoes the batch into a
        // fresh reference-sized table (2 * new_in_second), with the counters as they were
        if (debug_on() && same)
            std::fprintf(stderr, "reuse: %s, redo\n", ovf ? "level 2 overflowed" : "table region overflowed");
        HIPCHK(c, hipMemcpyAsync(c->d_ctr, &before, sizeof(before), hipMemcpyHostToDevice, s));
        HIPCHK(c, hipStreamSynchronize(s));
        on.no_hand_back();  // (the call waited for s; the ordinary pass joins again)
        return alloc_table(c, c->min_slots);
    }
    own_after_write(c, true, c->table_fresh);
    c->table_fresh = false;
    c->table_zero_pending = false;  // the fresh level 3 wrote every region
    c->n_chunks += b.size();
    c->n_bytes += bytes;
    c->reuse_hits++;
    c->reuse_last_level = c->reuse_level;
    if (c->profiling) on.prof.commit();
    if ((rc = on.hand_back())) return rc;
    *done = true;
    return KC_OK;
}

// The deferred level 3's group size for a counting pass over chunks (device_pass splits them into
// batches of batch_bytes / max_chunks): the batches' largest symbol bound fixes the segment
// geometry of every slot (part_plan, level-2 records of level2_record_bytes); a group takes as many
// batches as 90 % of the HBM left beside the level-1 buffers and the skew list (free + the
// partition buffers held now, less 2 GiB) holds level-2 slots for, at most MAX_SEG_GROUP segments
// per region.  The pass then runs partitioned when one sweep of the table per group beats the
// direct inserts (use_partitioned's rule with the table's bytes spread over the group), e.g. C5's
// one-GPU job, whose table is too large for a sweep per batch.  KC_DEFER=0: off.
static int plan_deferral_nb(kc_ctx* c, uint64_t nb, uint64_t syms);

static int plan_deferral(kc_ctx* c, const kc_chunk* chunks, size_t n) {
    uint64_t nb = 0, syms = 0, used = 0, cnt = 0;
    for (size_t i = 0; i <= n; i++) {
        const bool end = i == n;
        const uint64_t need = end ? 0 : round_up(chunks[i].len, TILE);
        if (!end && chunks[i].len == 0) continue;
        if (end || used + need > c->batch_bytes || cnt + 1 > c->max_chunks) {
            if (cnt) {
                nb++;
                syms = std::max(syms, used + cnt);
            }
            used = cnt = 0;
        }
        used += need;
        cnt++;
    }
    return plan_deferral_nb(c, nb, syms);
}

// (nb batches of at most syms symbols each)
static int plan_deferral_nb(kc_ctx* c, uint64_t nb, uint64_t syms) {
    // KC_DEFER: 0 = off, N = groups of at most N batches (tests)
    const char* kd = std::getenv("KC_DEFER");
    const uint64_t kmax = kd ? std::strtoull(kd, nullptr, 10) : ~0ULL;
    if (kmax == 0 || !c->nbuckets || !c->seg_ok) {
        if (debug_on()) std::fprintf(stderr, "deferred level 3: off (knob %d, table %d, segmented levels %d)\n",
                                     kmax != 0, c->nbuckets != 0, (int)c->seg_ok);
        return KC_OK;
    }
    const PathKnob pk = insert_path_knob();
    if (pk == PathKnob::Direct || pk == PathKnob::Exact) return KC_OK;
    if (nb < 2) return KC_OK;
    const PartPlan p = part_plan(c, syms, true, table_geo(c), 0, 1, 0, true);
    if (p.cap1 == 0) {
        if (debug_on()) std::fprintf(stderr, "deferred level 3: off (exact layout for this batch size)\n");
        return KC_OK;
    }
    const uint64_t rec2 = level2_record_bytes(c->W, c->cfg.k, c->R);
    const double slot_bytes = (double)c->R * p.B2 * p.cap2 * rec2;
    size_t fr = 0, tot = 0;
    HIPCHK(c, hipMemGetInfo(&fr, &tot));
    const double held = (double)(c->d_keys1.capacity() + c->d_keys2.capacity() + c->d_spill.capacity()) * 8.0;
    const double fixed =
        (double)(std::max(p.need1, c->d_keys1.capacity()) + std::max(p.spill_words, c->d_spill.capacity())) * 8.0;
    const double avail = 0.9 * ((double)fr + held - fixed) - (double)(2ull << 30);
    uint64_t g = avail > 0 ? (uint64_t)(avail / slot_bytes) : 0;
    g = std::min<uint64_t>({g, kmax, nb, MAX_SEG_GROUP / std::max<uint32_t>(1, p.B2),
                            ((1ULL << 31) - 1) / ((uint64_t)p.B2 * p.cap2)});
    // per batch: the direct inserts against the levels' key traffic + the group's table sweep
    const double table_bytes = (double)c->nbuckets * 128.0;
    const bool part_wins = pk == PathKnob::Partitioned || use_partitioned(c, syms) ||
                           (g >= 2 && (double)syms * 275.0 > (double)syms * (4.0 * c->W + 1) * 8.0 +
                                                                  2.0 * table_bytes / (double)g);
    if (debug_on())
        std::fprintf(stderr,
                     "deferred level 3: %llu batches, slot %.2f GB (%llu-byte records), free %.1f GB -> groups of "
                     "%llu%s\n",
                     (unsigned long long)nb, slot_bytes / 1e9, (unsigned long long)rec2, fr / 1e9,
                     (unsigned long long)g, part_wins ? "" : " (direct inserts cheaper: off)");
    if (g < 2 || !part_wins) return KC_OK;
    c->defer_on = true;
    c->defer_g = (uint32_t)g;
    c->defer_syms = syms;
    return KC_OK;
}

// Every exit of a pass (an error inside it included) ends its deferral; an error that leaves a
// group's batches counted without their level 3 marks the job broken
struct DeferEnd {
    kc_ctx* c;
    ~DeferEnd() {
        if (c->defer_on && c->defer_n > 0 && c->broken.empty())
            c->broken = "a counting pass failed with " + std::to_string(c->defer_n) +
                        " batch(es) of a deferred group not inserted: " + c->err;
        c->defer_on = c->defer_last = false;
        c->defer_n = 0;
        c->skew_prev = c->heavy_prev = 0;
    }
};

int device_pass(kc_ctx* c, const uint8_t* img, const kc_chunk* chunks, size_t n, int fmt, int pass,
                       hipStream_t s) {
    if (fmt != KC_FMT_FASTA && fmt != KC_FMT_FASTQ && fmt != KC_FMT_PLAIN) return c->fail(KC_ERR_ARG, "unknown format");
    int rc = flush_host(c);  // keep order with staged host chunks
    if (rc) return rc;
    StreamScope on(c, s);
    if ((rc = on.join())) return rc;
    std::vector<ChunkDesc> batch;
    uint64_t used = 0;
    // one staging batch holds the whole image?  (every chunk is checked before any is counted: a
    // pass either fails before its first batch or runs to its end)
    bool single = false;
    {
        uint64_t tot = 0, cnt = 0;
        for (size_t i = 0; i < n; i++)
            if (chunks[i].len) {
                if (round_up(chunks[i].len, TILE) > c->batch_bytes)
                    return c->fail(KC_ERR_ARG, "chunk larger than the staging batch");
                tot += round_up(chunks[i].len, TILE);
                cnt++;
            }
        single = cnt > 0 && tot <= c->batch_bytes && cnt <= c->max_chunks;
    }
    DeferEnd defer_end{c};
    // level-1 reuse: the Bloom pass keeps its level-1 output if it is the job's only batch
    const bool keep = pass == 1 && c->bloom_batches == 0 && reuse_enabled() && single;
    // the estimate pass's tokenized batches (kc_estimate_distinct_device), if this counting pass reads
    // the same image, chunks and format: used once, then dropped
    bool use_kept = false;
    if (c->kept_valid && pass == 0 && img == c->kept_img && fmt == c->kept_fmt && n == c->kept_chunks.size()) {
        use_kept = true;
        for (size_t i = 0; i < n && use_kept; i++)
            use_kept = chunks[i].off == c->kept_chunks[i].off && chunks[i].len == c->kept_chunks[i].len &&
                       chunks[i].broken_header == c->kept_chunks[i].broken_header;
    }
    if (pass != 3) c->kept_valid = false;
    size_t kept_i = 0;
    // (a pass over kept batches sizes its partition levels for their windows per symbol)
    struct Density {
        kc_ctx* c;
        double d;
        ~Density() { c->win_density = d; }
    } restore_density{c, c->win_density};
    if (use_kept) c->win_density = c->kept_density;
    // a counting pass of several batches defers level 3 (kc_ctx defer_*) when the segmented levels
    // run and HBM holds at least two batches' level-2 segments beside everything else
    c->defer_on = false;
    c->defer_n = 0;
    c->skew_prev = c->heavy_prev = 0;
    if (pass == 0 && !single) {
        rc = plan_deferral(c, chunks, n);
        if (rc) return rc;
    }
    bool last = false;
    auto launch = [&]() -> int {
        if (batch.empty()) return KC_OK;
        // descriptors go through the (idle) pinned desc buffer of the current slot
        std::memcpy(c->h_desc[c->cur], batch.data(), batch.size() * sizeof(ChunkDesc));
        HIPCHK(c, hipMemcpyAsync(c->d_chunks, c->h_desc[c->cur], batch.size() * sizeof(ChunkDesc),
                                 hipMemcpyHostToDevice, s));
        HIPCHK(c, hipEventRecord(c->h_free[c->cur], s));
        ProfEvents prof(c);
        const bool timed = c->profiling && pass != 3 && pass != 4;  // (the sketch / routing passes are not timed)
        if (timed) {
            prof.take(0);
            prof.take(1);
            HIPCHK(c, hipEventRecord(prof.ev[0], s));
        }
        // the image is tokenized in place (no gather into the stage): "gather" is ~0
        if (timed) HIPCHK(c, hipEventRecord(prof.ev[1], s));
        // the checksum of a batch the Bloom pass may keep (what a counting pass must present
        // again) runs on a second stream beside the pass's levels: both only read the image
        // (C3: 0.31 ms of streaming hidden under the latency-bound level 1)
        if (keep) {
            if (!c->aux) {
                HIPCHK(c, hipStreamCreateWithFlags(&c->aux, hipStreamNonBlocking));
                for (auto& e : c->aev) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
            }
            uint64_t max_len = 0;
            for (auto& d : batch) max_len = std::max<uint64_t>(max_len, d.len);
            HIPCHK(c, hipEventRecord(c->aev[0], s));
            HIPCHK(c, hipStreamWaitEvent(c->aux, c->aev[0], 0));
            HIPCHK(c, launch_checksum(img, c->d_chunks, (int)batch.size(), max_len, c->d_sum, c->aux));
            HIPCHK(c, hipEventRecord(c->aev[1], c->aux));
        }
        // the host gate of the batch's tail (the call waits for the batch) only for a one-batch
        // image; the batches of a larger image keep the device gate (kc_api.h: kc_count_device)
        // -- or a deferred pass, which reads each batch's flags
        c->defer_last = last;
        int r;
        if (use_kept && kept_i < c->kept.size()) {
            const PackedView kv{c->keep_pk + c->kept[kept_i].first, c->keep_bk + c->kept[kept_i].first};
            r = run_batch(c, img, c->kept[kept_i].second, 0, fmt, pass, s, &prof, keep, single, &kv,
                          c->d_kept_len + kept_i);
            kept_i++;
        } else {
            r = run_batch(c, img, used, batch.size(), fmt, pass, s, &prof, keep, single);
        }
        if (keep) HIPCHK(c, hipStreamWaitEvent(s, c->aev[1], 0));  // (before an error return, too)
        if (r) return r;
        if (keep && c->reuse_kept) {
            c->reuse_img = img;
            c->reuse_chunks = batch;
            c->reuse_fmt = fmt;
            c->reuse_used = used;
        }
        HIPCHK(c, hipEventSynchronize(c->h_free[c->cur]));
        batch.clear();
        used = 0;
        return KC_OK;
    };
    for (size_t i = 0; i < n; i++) {
        const uint64_t need = round_up(chunks[i].len, TILE);
        if (chunks[i].len == 0) continue;
        if (used + need > c->batch_bytes || batch.size() + 1 > c->max_chunks) {
            rc = launch();
            if (rc) return rc;
        }
        ChunkDesc d;
        d.src_off = chunks[i].off;
        d.stage_off = used;
        d.len = chunks[i].len;
        d.bh = chunks[i].broken_header ? 1 : 0;
        d.pad = 0;
        batch.push_back(d);
        used += need;
        if (pass == 0) { c->n_chunks++; c->n_bytes += chunks[i].len; }
    }
    last = true;
    rc = launch();
    if (rc) return rc;
    return on.finish();
}

extern "C" {

int kc_bloom_chunk(kc_ctx* c, const uint8_t* buf, size_t len, int fmt, int bh) {
    if (!c) return KC_ERR_ARG;
    JOB_OK(c);
    if (!c->cfg.bf_enable || c->bloom_final) return c->fail(KC_ERR_STATE, "bloom pass not active");
    return add_host_chunk(c, buf, len, fmt, bh, 1);
}

int kc_bloom_device(kc_ctx* c, const uint8_t* img, const kc_chunk* chunks, size_t n, int fmt, void* s) {
    if (!c || (!img && n) || (!chunks && n)) return KC_ERR_ARG;
    JOB_OK(c);
    if (!c->cfg.bf_enable || c->bloom_final) return c->fail(KC_ERR_STATE, "bloom pass not active");
    return device_pass(c, img, chunks, n, fmt, 1, (hipStream_t)s);
}

int kc_bloom_finalize(kc_ctx* c, uint64_t* new_in_second) {
    if (!c) return KC_ERR_ARG;
    if (!c->cfg.bf_enable || c->bloom_final) return c->fail(KC_ERR_STATE, "bloom pass not active");
    int rc = flush_host(c);
    if (rc) return rc;
    HIPCHK(c, hipDeviceSynchronize());
    DevCounters h;
    HIPCHK(c, hipMemcpy(&h, c->d_ctr, sizeof(h), hipMemcpyDeviceToHost));
    if (new_in_second) *new_in_second = h.new_in_second;
    c->bloom_final = true;
    // partition reuse: the only Bloom batch kept its partitions and no key of them went to a
    // skew list.  The table then takes power-of-two hash-prefix bins: R_t regions with the
    // fine geometry's coarse bins (F1); from level 2 if its regions are unions of fine bins
    // (R_t <= R_fine, at most MAX_SEG_GROUP segments per region), else from level 1 if that
    // level 2 fits the LDS.
    bool reuse = c->reuse_kept && c->bloom_batches == 1 && h.part_fallbacks == 0 && h.spilled == 0 && h.heavy == 0;
    const uint64_t slots = 2 * h.new_in_second;  // main.cpp:454
    c->reuse_level = 0;
    if (reuse) {
        uint64_t want = std::max<uint64_t>(slots, 64);
        want += want / 4;
        const uint64_t regions = std::max<uint64_t>(1, ((want + c->S - 1) / c->S + BPR - 1) / BPR);
        uint64_t rt = c->fgeo.F1;
        while (rt < regions) rt *= 2;
        const uint32_t nseg = (c->pbf.nblk1 + c->pbf.B2 - 1) / std::max<uint32_t>(1, c->pbf.B2);
        if (rt <= c->fgeo.R && (c->fgeo.R / rt) * c->pbf.B2 <= MAX_SEG_GROUP)
            c->reuse_level = 2;
        else if (p2f_lds_bytes(c->W, (uint32_t)(rt / c->fgeo.F1), nseg) <= 160 * 1024 && rt < (1ULL << 32))
            c->reuse_level = 1;
        reuse = c->reuse_level != 0;
        // adaptive fine geometry for the context's next job (kc_reset applies it): fine
        // bins as coarse as the table regions just sized, so that a level-2 region is one
        // fine bin (one segment group per k_p3 workgroup, fewer and fuller level-2 bins:
        // C3 31.3 -> 29.4 ms, profiles/r03_ab_fb16.txt); back to the create-time geometry
        // when this job's table outgrew the learned one.  The first job keeps the default.
        const uint64_t floor_r = std::max<uint64_t>(c->bgeo.R, c->fgeo.F1);
        if (c->reuse_level == 2)
            c->fgeo_next_R = std::max(rt, floor_r);
        else if (rt > c->fgeo.R && c->fgeo.R < c->fgeo_max_R)
            c->fgeo_next_R = c->fgeo_max_R;
    }
    if (reuse) {
        unsigned long long part[CHECKSUM_SLOTS];
        HIPCHK(c, hipMemcpy(part, c->d_sum, sizeof(part), hipMemcpyDeviceToHost));
        c->reuse_sum = 0;
        for (auto v : part) c->reuse_sum += v;
        c->reuse_windows = h.bf_windows;
    }
    c->reuse_ok = reuse;
    if (debug_on())
        std::fprintf(stderr, "reuse finalize: kept %d batches %d fallbacks %llu spilled %llu heavy %llu -> level %d\n",
                     (int)c->reuse_kept, c->bloom_batches, (unsigned long long)h.part_fallbacks,
                     (unsigned long long)h.spilled, (unsigned long long)h.heavy, c->reuse_level);
    rc = alloc_table(c, slots, reuse ? c->fgeo.F1 : 0);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KC_OK;
}

int kc_count_chunk(kc_ctx* c, const uint8_t* buf, size_t len, int fmt, int bh) {
    if (!c) return KC_ERR_ARG;
    JOB_OK(c);
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "kc_bloom_finalize must precede the counting pass");
    return add_host_chunk(c, buf, len, fmt, bh, 0);
}

int kc_count_device(kc_ctx* c, const uint8_t* img, const kc_chunk* chunks, size_t n, int fmt, void* s) {
    if (!c || (!img && n) || (!chunks && n)) return KC_ERR_ARG;
    JOB_OK(c);
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "kc_bloom_finalize must precede the counting pass");
    if (c->reuse_ok) {  // one chance: the first counting pass after the Bloom pass
        c->reuse_ok = false;
        bool done = false;
        const int rc = count_reused(c, img, chunks, n, fmt, (hipStream_t)s, &done);
        if (rc || done) return rc;
    }
    return device_pass(c, img, chunks, n, fmt, 0, (hipStream_t)s);
}

int kc_estimate_distinct_device(kc_ctx* c, const uint8_t* img, const kc_chunk* chunks, size_t n, int fmt, void* sp,
                                double* estimate) {
    if (!c || !estimate || (!img && n) || (!chunks && n)) return KC_ERR_ARG;
    hipStream_t s = (hipStream_t)sp;
    if (!c->d_hll.reserve(HLL_M))
        return c->fail(KC_ERR_NOMEM, "sketch allocation failed");
    HIPCHK(c, hipMemsetAsync(c->d_hll, 0, HLL_M * 4, s));
    // the tokenized batches are kept for the counting pass when they take < 1/8 of the free HBM
    c->kept_valid = false;
    c->kept.clear();
    c->keep_woff = 0;
    c->keep_target = false;
    {
        uint64_t words = 64;
        for (size_t i = 0; i < n; i++) words += (round_up(chunks[i].len, TILE) + 1) / 32 + 5;
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) {
            const uint64_t keep_cap = c->keep_pk.capacity();
            if (words > keep_cap && (double)words * 12 < (double)(fr + keep_cap * 12) / 8)
                (void)reserve_pair(c->keep_pk, words, c->keep_bk, words);
            (void)reserve_pair(c->d_kept_len, 8192, c->d_kept_win, 8192);
            c->keep_target = c->keep_pk.capacity() >= words && c->d_kept_len.capacity() > 0;
        }
    }
    HIPCHK(c, hipMemsetAsync(&c->d_ctr->est_windows, 0, 8, s));
    int rc = device_pass(c, img, chunks, n, fmt, 3, s);
    const bool kept = c->keep_target;
    c->keep_target = false;
    if (rc) return rc;
    if (kept) {
        // the kept batches' windows per symbol: the counting pass sizes its segments for them (a batch
        // of 150 bp reads holds 0.62 windows per symbol at k = 51; sized per symbol, C4's deferred
        // level-2 slots were 2.1 x its records and a pass took two groups)
        std::vector<uint64_t> wins(c->kept.size()), lens(c->kept.size());
        HIPCHK(c, hipMemcpyAsync(wins.data(), c->d_kept_win, wins.size() * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipMemcpyAsync(lens.data(), c->d_kept_len, lens.size() * 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        double d = 0;
        for (size_t i = 0; i < wins.size(); i++) {
            const uint64_t w = wins[i] - (i ? wins[i - 1] : 0);
            d = std::max(d, (double)w / (double)std::max<uint64_t>(1, lens[i]));
        }
        c->kept_density = std::min(1.0, d * 1.02 + 0.005);
        c->kept_valid = true;
        c->kept_img = img;
        c->kept_fmt = fmt;
        c->kept_chunks.assign(chunks, chunks + n);
    }
    std::vector<uint32_t> reg(HLL_M);
    HIPCHK(c, hipMemcpyAsync(reg.data(), c->d_hll, HLL_M * 4, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    // Flajolet et al. 2007: E = alpha_m m^2 / sum 2^-M[j]; linear counting m ln(m / V) below
    // 2.5 m when V registers are empty (a 64-bit hash needs no large-range correction)
    double sum = 0;
    uint32_t zeros = 0;
    for (uint32_t v : reg) {
        sum += std::ldexp(1.0, -(int)v);
        zeros += v == 0;
    }
    const double m = HLL_M, alpha = 0.7213 / (1.0 + 1.079 / m);
    double e = alpha * m * m / sum;
    if (e <= 2.5 * m && zeros) e = m * std::log(m / zeros);
    *estimate = std::ldexp(e, hll_sample_bits(c->W));  // (k_hll_s: the sample's estimate)
    return KC_OK;
}

// A symbol stream in HBM (a received super-k-mer stream) through the pass's levels in batches of
// about a staging batch's windows, cut at words whose first symbol is a break (no window spans a
// cut), with the deferred level 3 of a counting pass over several batches.  `windows` is the
// caller's hint and only chooses the cut length (packed_cut_words); the buffers are sized from the
// windows counted in each batch (k_packed_windows: one read of the batches' break words and one
// host wait per pass), since the exact pipeline writes every window of a batch unchecked and a
// stream need not be uniform (kc_plan_host.h packed_batch_density).
static int packed_pass(kc_ctx* c, const uint64_t* pk, const uint32_t* bk, uint64_t n_words, uint64_t windows, int pass,
                       hipStream_t s) {
    int rc = flush_host(c);  // keep order with staged host chunks
    if (rc) return rc;
    StreamScope on(c, s);
    if ((rc = on.join())) return rc;
    if (n_words == 0) {
        on.no_hand_back();  // (nothing ran on s)
        return KC_OK;
    }
    const uint64_t lim = packed_cut_words(c->batch_bytes, n_words, windows);
    std::vector<uint64_t> cuts{0};
    std::vector<uint32_t> probe(4096);
    while (n_words - cuts.back() > lim) {
        uint64_t w = cuts.back() + lim;
        bool found = false;
        while (!found && w < n_words) {
            const uint64_t m = std::min<uint64_t>(probe.size(), n_words - w);
            HIPCHK(c, hipMemcpyAsync(probe.data(), bk + w, m * 4, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
            uint64_t i = 0;
            while (i < m && !(probe[i] >> 31)) i++;
            w += i;
            found = i < m;
        }
        if (!found) break;
        cuts.push_back(w);
    }
    cuts.push_back(n_words);
    const uint64_t nb = cuts.size() - 1;
    uint64_t maxs = 0;
    for (uint64_t i = 0; i < nb; i++) maxs = std::max<uint64_t>(maxs, (cuts[i + 1] - cuts[i]) * 32);
    // every batch's windows, counted; the pass plans at the largest windows per symbol of a batch
    std::vector<unsigned long long> bw(nb);
    if (!c->d_pwin.reserve(nb)) return c->fail(KC_ERR_NOMEM, "window count allocation failed");
    HIPCHK(c, hipMemsetAsync(c->d_pwin, 0, nb * 8, s));
    for (uint64_t i = 0; i < nb; i++)
        HIPCHK(c, launch_packed_windows(bk + cuts[i], cuts[i + 1] - cuts[i], c->cfg.k, c->d_pwin + i, s));
    HIPCHK(c, hipMemcpyAsync(bw.data(), c->d_pwin, nb * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    double measured = 0;
    for (uint64_t i = 0; i < nb; i++)
        measured = std::max(measured, packed_batch_density(bw[i], (cuts[i + 1] - cuts[i]) * 32));
    const double dens = packed_plan_density(packed_hint_density(n_words, windows), measured);
    struct Density {
        kc_ctx* c;
        double d;
        ~Density() { c->win_density = d; }
    } restore{c, c->win_density};
    c->win_density = dens;
    DeferEnd defer_end{c};
    c->defer_on = false;
    c->defer_n = 0;
    c->skew_prev = c->heavy_prev = 0;
    if (pass == 0 && nb >= 2 && (rc = plan_deferral_nb(c, nb, maxs))) return rc;
    for (uint64_t i = 0; i < nb; i++) {
        c->defer_last = i + 1 == nb;
        const PackedView v{const_cast<uint64_t*>(pk) + cuts[i], const_cast<uint32_t*>(bk) + cuts[i]};
        if ((rc = run_batch(c, nullptr, (cuts[i + 1] - cuts[i]) * 32, 0, 0, pass, s, nullptr, false, nb == 1,
                            &v)))
            return rc;
    }
    return on.finish();
}

int kc_count_packed_device(kc_ctx* c, const uint64_t* pk, const uint32_t* bk, uint64_t n_words, uint64_t windows,
                           void* sp) {
    if (!c || (n_words && (!pk || !bk))) return KC_ERR_ARG;
    JOB_OK(c);
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "kc_bloom_finalize must precede the counting pass");
    c->reuse_ok = false;  // (the Bloom pass's kept partitions are an image's)
    return packed_pass(c, pk, bk, n_words, windows, 0, (hipStream_t)sp);
}

int kc_packed_windows_device(kc_ctx* c, const uint64_t* pk, const uint32_t* bk, uint64_t n_words, void* sp,
                             uint64_t* windows) {
    (void)pk;  // (the windows of a stream depend on its breaks alone)
    if (!c || !windows || (n_words && !bk)) return KC_ERR_ARG;
    *windows = 0;
    if (n_words == 0) return KC_OK;
    hipStream_t s = (hipStream_t)sp;
    if (!c->d_pwin.reserve(1)) return c->fail(KC_ERR_NOMEM, "window count allocation failed");
    unsigned long long n = 0;
    HIPCHK(c, hipMemsetAsync(c->d_pwin, 0, 8, s));
    HIPCHK(c, launch_packed_windows(bk, n_words, c->cfg.k, c->d_pwin, s));
    HIPCHK(c, hipMemcpyAsync(&n, c->d_pwin, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    *windows = n;
    return KC_OK;
}

int kc_bloom_packed_device(kc_ctx* c, const uint64_t* pk, const uint32_t* bk, uint64_t n_words, uint64_t windows,
                           void* sp) {
    if (!c || (n_words && (!pk || !bk))) return KC_ERR_ARG;
    JOB_OK(c);
    if (!c->cfg.bf_enable || c->bloom_final) return c->fail(KC_ERR_STATE, "bloom pass not active");
    return packed_pass(c, pk, bk, n_words, windows, 1, (hipStream_t)sp);
}

}  // extern "C"
