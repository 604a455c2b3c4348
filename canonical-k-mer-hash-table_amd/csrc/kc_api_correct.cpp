// kc_api_correct.cpp -- read correction from the counted table (include/kc_api.h kc_correct*): per
// pass the per-position counts of the sequence queries (kc_seq.hip, kc_seq_impl.h), then mark, try
// and apply (kc_correct.hip, kc_correct_impl.h).
#include "kc_ctx.h"

extern "C" {

int kc_correct_device(kc_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t n_seqs,
                      uint32_t solid_min, uint8_t* out, kc_correct_stat* stats, void* sp) {
    if (!c) return KC_ERR_ARG;
    if (n_seqs && !offsets) return c->fail(KC_ERR_ARG, "null offsets");
    for (uint64_t i = 0; i < n_seqs; i++)
        if (offsets[i] > offsets[i + 1]) return c->fail(KC_ERR_ARG, "sequence offsets decrease");
    if (n_seqs && offsets[n_seqs] > n) return c->fail(KC_ERR_ARG, "sequence offsets pass the end of the text");
    if (n && (!text || !out)) return c->fail(KC_ERR_ARG, "null text or output");
    if (n && out != text && out < text + n && text < out + n)
        return c->fail(KC_ERR_ARG, "the output overlaps the text (only out == text is allowed)");
    JOB_OK(c);
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table (kc_bloom_finalize must precede a correction)");
    if (n == 0) return KC_OK;
    hipStream_t s = (hipStream_t)sp;
    int rc;
    if ((rc = flush_host(c))) return rc;
    StreamScope on(c, s);
    if ((rc = on.join())) return rc;
    if ((rc = materialize_zero(c, s))) return rc;  // an emptied table answers 0: nothing is solid
    const uint64_t k = (uint64_t)c->cfg.k;
    const uint64_t t0 = n_seqs ? offsets[0] : n, t1 = n_seqs ? offsets[n_seqs] : n;
    if (out != text) {  // the bytes outside the sequences
        if (t0) HIPCHK(c, hipMemcpyAsync(out, text, t0, hipMemcpyDeviceToDevice, s));
        if (t1 < n) HIPCHK(c, hipMemcpyAsync(out + t1, text + t1, n - t1, hipMemcpyDeviceToDevice, s));
    }
    if (stats && n_seqs) HIPCHK(c, hipMemsetAsync(stats, 0, n_seqs * sizeof(kc_correct_stat), s));
    if (t1 == t0) return on.finish();
    // passes: whole sequences of at most batch_bytes together (one longer sequence: a pass of its own)
    struct Pass { uint64_t i0, i1; };
    std::vector<Pass> passes;
    uint64_t max_len = 0;
    for (uint64_t i = 0; i < n_seqs;) {
        Pass p{i, i + 1};
        while (p.i1 < n_seqs && offsets[p.i1 + 1] - offsets[i] <= c->batch_bytes) p.i1++;
        max_len = std::max(max_len, offsets[p.i1] - offsets[i]);
        passes.push_back(p);
        i = p.i1;
    }
    // the offsets go through pinned memory of the context, as kc_seq_stats_device's do
    const uint64_t n_off = n_seqs + 1;
    if (!c->seq_ev) HIPCHK(c, hipEventCreateWithFlags(&c->seq_ev, hipEventDisableTiming));
    HIPCHK(c, hipEventSynchronize(c->seq_ev));
    const uint64_t nw = seq_pack_words(max_len);
    if (c->d_seq_cnt.capacity() < max_len || c->d_cor_vd.capacity() < max_len || c->d_seq_off.capacity() < n_off ||
        c->d_seq_pk.capacity() < nw || c->d_seq_bk.capacity() < nw)
        make_room(c, max_len * 5 + nw * 12 + n_off * 8);
    if (!c->h_seq_off.reserve(n_off) || !c->d_seq_off.reserve(n_off) || !c->d_seq_cnt.reserve(max_len) ||
        !c->d_cor_vd.reserve(max_len) || !reserve_pair(c->d_seq_pk, nw, c->d_seq_bk, nw))
        return c->fail(KC_ERR_NOMEM, "read correction: scratch allocation failed");
    std::memcpy(c->h_seq_off, offsets, n_off * 8);
    HIPCHK(c, hipMemcpyAsync(c->d_seq_off, c->h_seq_off, n_off * 8, hipMemcpyHostToDevice, s));
    HIPCHK(c, hipEventRecord(c->seq_ev, s));
    const PackedView sv{c->d_seq_pk, c->d_seq_bk};
    const int count_mode = c->cfg.mode == 0 ? 0 : 1;
    const uint32_t smin = std::max<uint32_t>(solid_min, 1);
    for (const Pass& p : passes) {
        const uint64_t l0 = offsets[p.i0], len = offsets[p.i1] - l0;
        if (len < k) {  // no window: no candidate
            if (len && out != text) HIPCHK(c, hipMemcpyAsync(out + l0, text + l0, len, hipMemcpyDeviceToDevice, s));
            continue;
        }
        HIPCHK(c, launch_seq_pack(text + l0, len, sv, s));
        HIPCHK(c, launch_seq_counts(table_view(c), sv, c->cfg.k, count_mode, len, len, c->d_seq_cnt, s));
        HIPCHK(c, launch_correct_mark(c->d_seq_cnt, len, l0, c->d_seq_off, p.i0, p.i1, c->cfg.k, smin, c->d_cor_vd, s));
        HIPCHK(c, launch_correct_try(table_view(c), sv, c->d_seq_cnt, len, l0, c->d_seq_off, p.i0, p.i1, c->cfg.k,
                                     count_mode, smin, c->d_cor_vd, s));
        HIPCHK(c, launch_correct_apply(text + l0, out + l0, c->d_cor_vd, len, l0, c->d_seq_off, p.i0, p.i1, c->cfg.k,
                                       stats, s));
    }
    return on.finish();
}

int kc_correct(kc_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t n_seqs,
               uint32_t solid_min, uint8_t* out, kc_correct_stat* stats) {
    if (!c) return KC_ERR_ARG;
    if (n_seqs && !offsets) return c->fail(KC_ERR_ARG, "null offsets");
    if (n && (!text || !out)) return c->fail(KC_ERR_ARG, "null text or output");
    if (n && out != text && out < text + n && text < out + n)
        return c->fail(KC_ERR_ARG, "the output overlaps the text (only out == text is allowed)");
    DevBuf<uint8_t> dt;  // corrected in place on the device
    DevBuf<kc_correct_stat> ds;
    const bool want = stats && n_seqs;
    if (n) {
        JOB_OK(c);
        if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table (kc_bloom_finalize must precede a correction)");
        make_room(c, n + n_seqs * sizeof(kc_correct_stat));
        if (!dt.reserve(n) || (want && !ds.reserve(n_seqs))) return c->fail(KC_ERR_NOMEM, "read correction buffers");
    }
    hipError_t e = n ? hipMemcpyAsync(dt, text, n, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    int rc = e == hipSuccess ? kc_correct_device(c, dt, n, offsets, n_seqs, solid_min, dt, want ? ds.get() : nullptr, c->stream)
                             : c->hipfail(e, "read correction: text copy");
    if (rc == KC_OK && n) {
        e = hipMemcpyAsync(out, dt, n, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && want)
            e = hipMemcpyAsync(stats, ds, n_seqs * sizeof(kc_correct_stat), hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = c->hipfail(e, "read correction: result copy");
    } else {
        (void)hipStreamSynchronize(c->stream);  // (the text copy writes dt)
        // n_bytes = 0: every sequence is empty
        if (rc == KC_OK && stats && n_seqs) std::memset(stats, 0, n_seqs * sizeof(kc_correct_stat));
    }
    return rc;
}

}  // extern "C"
