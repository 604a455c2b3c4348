// kc_api_seq.cpp -- sequence queries of the counted table (include/kc_api.h): the count of the
// k-mer at every position of a text (kc_text_counts*) and per-sequence statistics of those counts
// (kc_seq_stats*).  Kernels: kc_seq.hip (pack, reduce) and kc_seq_impl.h (the fused count kernel).
#include "kc_ctx.h"

#pragma GCC visibility push(hidden)

// what every entry point checks before it touches the device
static int seq_ready(kc_ctx* c) {
    JOB_OK(c);
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table (kc_bloom_finalize must precede a sequence query)");
    return KC_OK;
}

// the packed stream of a pass of up to n bytes (3/8 byte per byte)
int seq_stream_bufs(kc_ctx* c, uint64_t n) {
    const uint64_t nw = seq_pack_words(n);
    if (c->d_seq_pk.capacity() < nw || c->d_seq_bk.capacity() < nw) make_room(c, nw * 12);
    if (!reserve_pair(c->d_seq_pk, nw, c->d_seq_bk, nw))
        return c->fail(KC_ERR_NOMEM, "sequence query: packed stream allocation failed");
    return KC_OK;
}

// counts[p] for the n_pos positions from text on, of which n_sym >= n_pos bytes are readable
static int seq_counts_pass(kc_ctx* c, const uint8_t* text, uint64_t n_pos, uint64_t n_sym, uint32_t* counts,
                           hipStream_t s) {
    const PackedView sv{c->d_seq_pk, c->d_seq_bk};
    if (n_sym >= (uint64_t)c->cfg.k) HIPCHK(c, launch_seq_pack(text, n_sym, sv, s));
    HIPCHK(c, launch_seq_counts(table_view(c), sv, c->cfg.k, c->cfg.mode == 0 ? 0 : 1, n_pos, n_sym, counts, s));
    return KC_OK;
}

#pragma GCC visibility pop

extern "C" {

int kc_text_counts_device(kc_ctx* c, const uint8_t* text, uint64_t n, uint32_t* counts, void* sp) {
    if (!c) return KC_ERR_ARG;
    if (n && (!text || !counts)) return c->fail(KC_ERR_ARG, "null text or count array");
    int rc = seq_ready(c);
    if (rc) return rc;
    if (n == 0) return KC_OK;
    hipStream_t s = (hipStream_t)sp;
    if ((rc = flush_host(c))) return rc;
    StreamScope on(c, s);
    if ((rc = on.join())) return rc;
    if ((rc = materialize_zero(c, s))) return rc;  // an emptied table answers 0
    // pieces of batch_bytes positions, so that the packed stream stays bounded; a piece's stream
    // runs k - 1 bytes on, to the end of its last window
    const uint64_t piece = c->batch_bytes, k1 = (uint64_t)c->cfg.k - 1;
    if ((rc = seq_stream_bufs(c, std::min(n, piece + k1)))) return rc;
    for (uint64_t p0 = 0; p0 < n; p0 += piece) {
        const uint64_t left = n - p0;
        if ((rc = seq_counts_pass(c, text + p0, std::min(left, piece), std::min(left, piece + k1), counts + p0, s)))
            return rc;
    }
    return on.finish();
}

int kc_text_counts(kc_ctx* c, const uint8_t* text, uint64_t n, uint32_t* counts) {
    if (!c) return KC_ERR_ARG;
    if (n && (!text || !counts)) return c->fail(KC_ERR_ARG, "null text or count array");
    int rc = seq_ready(c);
    if (rc) return rc;
    if (n == 0) return KC_OK;
    DevBuf<uint8_t> dt;
    DevBuf<uint32_t> dc;
    make_room(c, n * 5);
    if (!dt.reserve(n) || !dc.reserve(n)) return c->fail(KC_ERR_NOMEM, "text count buffers");
    hipError_t e = hipMemcpyAsync(dt, text, n, hipMemcpyHostToDevice, c->stream);
    rc = e == hipSuccess ? kc_text_counts_device(c, dt, n, dc, c->stream) : c->hipfail(e, "text counts: text copy");
    if (rc == KC_OK) {
        e = hipMemcpyAsync(counts, dc, n * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = c->hipfail(e, "text counts: count copy");
    } else {
        (void)hipStreamSynchronize(c->stream);  // (the text copy writes dt)
    }
    return rc;
}

int kc_seq_stats_device(kc_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t n_seqs,
                        uint32_t solid_min, kc_seq_stat* stats, void* sp) {
    if (!c) return KC_ERR_ARG;
    if (n_seqs && (!offsets || !stats)) return c->fail(KC_ERR_ARG, "null offsets or statistics array");
    for (uint64_t i = 0; i < n_seqs; i++)
        if (offsets[i] > offsets[i + 1]) return c->fail(KC_ERR_ARG, "sequence offsets decrease");
    if (n_seqs && offsets[n_seqs] > n) return c->fail(KC_ERR_ARG, "sequence offsets pass the end of the text");
    if (n_seqs && offsets[n_seqs] > offsets[0] && !text) return c->fail(KC_ERR_ARG, "null text");
    int rc = seq_ready(c);
    if (rc) return rc;
    if (n_seqs == 0) return KC_OK;
    hipStream_t s = (hipStream_t)sp;
    if ((rc = flush_host(c))) return rc;
    StreamScope on(c, s);
    if ((rc = on.join())) return rc;
    if ((rc = materialize_zero(c, s))) return rc;
    // passes: whole sequences of at most batch_bytes together (one longer sequence: a pass of its
    // own); the sequences of more than SEQ_WAVE_MAX bytes take the workgroup form of the reduction
    struct Pass { uint64_t i0, i1, long0, n_long; };
    std::vector<Pass> passes;
    std::vector<uint64_t> long_ids;
    uint64_t max_len = 0;
    for (uint64_t i = 0; i < n_seqs;) {
        Pass p{i, i + 1, long_ids.size(), 0};
        while (p.i1 < n_seqs && offsets[p.i1 + 1] - offsets[i] <= c->batch_bytes && p.i1 - i < (1ull << 30)) p.i1++;
        for (uint64_t j = i; j < p.i1; j++)
            if (offsets[j + 1] - offsets[j] > SEQ_WAVE_MAX) long_ids.push_back(j);
        p.n_long = long_ids.size() - p.long0;
        max_len = std::max(max_len, offsets[p.i1] - offsets[i]);
        passes.push_back(p);
        i = p.i1;
    }
    // the offsets and the long ids go through pinned memory of the context: the caller's array is
    // free once this call returns, and an earlier call's copy has read the block before it is reused
    const uint64_t n_off = n_seqs + 1, n_tab = n_off + long_ids.size();
    if (!c->seq_ev) HIPCHK(c, hipEventCreateWithFlags(&c->seq_ev, hipEventDisableTiming));
    HIPCHK(c, hipEventSynchronize(c->seq_ev));
    if (c->d_seq_cnt.capacity() < max_len || c->d_seq_off.capacity() < n_tab) make_room(c, max_len * 4 + n_tab * 8);
    if (!c->h_seq_off.reserve(n_tab) || !c->d_seq_off.reserve(n_tab) || !c->d_seq_cnt.reserve(std::max<uint64_t>(1, max_len)))
        return c->fail(KC_ERR_NOMEM, "sequence statistics: scratch allocation failed");
    if ((rc = seq_stream_bufs(c, max_len))) return rc;
    std::memcpy(c->h_seq_off, offsets, n_off * 8);
    if (!long_ids.empty()) std::memcpy(c->h_seq_off + n_off, long_ids.data(), long_ids.size() * 8);
    HIPCHK(c, hipMemcpyAsync(c->d_seq_off, c->h_seq_off, n_tab * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(c->seq_ev, s));
    for (const Pass& p : passes) {
        const uint64_t l0 = offsets[p.i0], len = offsets[p.i1] - l0;
        if (len >= (uint64_t)c->cfg.k && (rc = seq_counts_pass(c, text + l0, len, len, c->d_seq_cnt, s))) return rc;
        HIPCHK(c, launch_seq_reduce(c->d_seq_cnt, l0, c->d_seq_off, p.i0, p.i1, c->d_seq_off + n_off + p.long0, p.n_long,
                                    c->cfg.k, solid_min, stats, s));
    }
    return on.finish();
}

int kc_seq_stats(kc_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t n_seqs,
                 uint32_t solid_min, kc_seq_stat* stats) {
    if (!c) return KC_ERR_ARG;
    if (n_seqs && (!offsets || !stats)) return c->fail(KC_ERR_ARG, "null offsets or statistics array");
    if (n && !text) return c->fail(KC_ERR_ARG, "null text");
    int rc = seq_ready(c);
    if (rc) return rc;
    if (n_seqs == 0) return KC_OK;
    DevBuf<uint8_t> dt;
    DevBuf<kc_seq_stat> ds;
    make_room(c, n + n_seqs * sizeof(kc_seq_stat));
    if (!dt.reserve(std::max<uint64_t>(1, n)) || !ds.reserve(n_seqs)) return c->fail(KC_ERR_NOMEM, "sequence statistics buffers");
    hipError_t e = n ? hipMemcpyAsync(dt, text, n, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    rc = e == hipSuccess ? kc_seq_stats_device(c, dt, n, offsets, n_seqs, solid_min, ds, c->stream)
                         : c->hipfail(e, "sequence statistics: text copy");
    if (rc == KC_OK) {
        e = hipMemcpyAsync(stats, ds, n_seqs * sizeof(kc_seq_stat), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = c->hipfail(e, "sequence statistics: result copy");
    } else {
        (void)hipStreamSynchronize(c->stream);  // (the text copy writes dt)
    }
    return rc;
}

}  // extern "C"
