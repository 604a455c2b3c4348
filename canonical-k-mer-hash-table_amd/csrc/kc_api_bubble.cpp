// kc_api_bubble.cpp -- bubble popping (include/kc_api.h kc_pop_bubbles*): the graph of src's range
// without the weaker of its parallel unitigs, added into dst as a counted table.  The ranking is
// kc_unitigs*'s (kc_api_unitig.cpp unitig_rank, on src's scratch, with one verdict byte and two
// anchors per id on top); kernels: k_bubble_anchors and k_bubble_verdict (kc_bubble_impl.h), then
// kc_clean*'s copy k_clean (kc_clean_impl.h) as it is.
#include "kc_ctx.h"

#pragma GCC visibility push(hidden)

static_assert(sizeof(kc_bubble_desc) == 24 && sizeof(kc_bubble_stats) == 64, "include/kc_api.h states these sizes");
static_assert(sizeof(kc_bubble_stats) == 8 * sizeof(unsigned long long) && offsetof(kc_bubble_stats, branches) == 2 * 8 &&
                  offsetof(kc_bubble_stats, parallel) == 3 * 8 && offsetof(kc_bubble_stats, out_keys) == 6 * 8,
              "k_bubble_anchors adds words 0-2, k_bubble_verdict words 3-5, k_clean words 6 and 7");
static_assert(UNITIG_NODE_BYTES + UNITIG_VERDICT_BYTES + UNITIG_ANCHOR_BYTES == 149,
              "include/kc_api.h states the scratch of kc_pop_bubbles*");

// W-dispatch of the two kernels (kc_bubble_w.hip, one translation unit per key width)
static hipError_t launch_bubble(TableView src, int k, UnitigBufs u, int rounds, uint32_t* anc, BubbleRule rule,
                                unsigned long long* stats, hipStream_t s) {
    KC_DISPATCH(BubbleOps, src.W, pop(src, k, u, rounds, anc, rule, stats, s));
}

// the error of a call on `from` is reported on the context the caller reads (dst, else src)
static int bubble_rc(kc_ctx* err, kc_ctx* from, int rc) {
    if (rc && from != err) err->err = from->err;
    return rc;
}

// what both forms check before they touch the device; err receives the message
static int bubble_check(kc_ctx* err, kc_ctx* dst, kc_ctx* src, const kc_bubble_desc* d) {
    if (dst == src) return err->fail(KC_ERR_ARG, "kc_pop_bubbles: dst must not be src");
    if (dst && (dst->cfg.k != src->cfg.k || dst->cfg.device != src->cfg.device))
        return err->fail(KC_ERR_ARG, "kc_pop_bubbles: the contexts must have the same k and device");
    if (d->reserved) return err->fail(KC_ERR_ARG, "kc_pop_bubbles: reserved must be 0");
    // k < 2, min_count above a non-zero max_count; then src's job and table
    int rc = bubble_rc(err, src, unitig_check(src, d->min_count, d->max_count));
    if (rc) return rc;
    if (dst) {
        if (!dst->broken.empty()) return err->fail(KC_ERR_STATE, dst->broken + " (kc_reset first)");
        if (!dst->nbuckets) return err->fail(KC_ERR_STATE, "no table (kc_bloom_finalize must precede a bubble popping)");
    }
    return KC_OK;
}

// The call on s with `bound` node ids (the caller has checked).  No host wait.
static int bubble_on(kc_ctx* err, kc_ctx* dst, kc_ctx* src, const kc_bubble_desc* d, uint64_t bound,
                     kc_bubble_stats* dev_stats, hipStream_t s) {
    int rc;
    for (kc_ctx* x : {dst, src})
        if (x && (rc = bubble_rc(err, x, flush_host(x)))) return rc;
    StreamScope on_s(src, s);
    if ((rc = bubble_rc(err, src, on_s.join()))) return rc;
    // an emptied src has no unitigs (and its memory is not read before it is zeroed)
    if ((rc = bubble_rc(err, src, materialize_zero(src, s)))) return rc;
    UnitigBufs u;
    int rounds = 0;
    // the scratch first: KC_ERR_NOMEM before any kernel of the call
    if ((rc = bubble_rc(err, src, unitig_rank(src, d->min_count, d->max_count, bound, s, &u, &rounds, false, true, true))))
        return rc;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(dev_stats);
    if (st) HIPCHK(err, hipMemsetAsync(st, 0, sizeof(kc_bubble_stats), s));
    const TableView ts = table_view(src);
    HIPCHK(err, launch_unitig_heads(u, src->cfg.k, rounds, nullptr, 0, 0, nullptr, s));
    HIPCHK(err, launch_bubble(ts, src->cfg.k, u, rounds, unitig_anchors(src, u),
                              BubbleRule{d->max_nodes, d->max_diff, d->max_mean}, st, s));
    auto work = [&]() -> int {
        HIPCHK(err, launch_clean(ts, dst ? table_view(dst) : TableView{}, u, dst ? dst->d_ctr.get() : nullptr, st, s));
        return KC_OK;
    };
    if (dst) {
        // dst's host-side state as after kc_table_op_device; the compact representation is a
        // snapshot of the table before this call
        if (dst->d_cwords) drop_compact(dst);
        StreamScope on_d(dst, s);
        rc = insert_on(dst, on_d, false, true, [&] { return materialize_zero(dst, s); }, work);
    } else {
        rc = work();
    }
    if (rc) return rc;
    return bubble_rc(err, src, on_s.finish());
}

#pragma GCC visibility pop

extern "C" {

int kc_pop_bubbles_device(kc_ctx* dst, kc_ctx* src, const kc_bubble_desc* d, kc_bubble_stats* dev_stats, void* sp) {
    kc_ctx* err = dst ? dst : src;
    if (!src || !d) return err ? err->fail(KC_ERR_ARG, "kc_pop_bubbles: null source or descriptor") : KC_ERR_ARG;
    int rc = bubble_check(err, dst, src, d);
    if (rc) return rc;
    // no host wait, so the ids are sized by what the host knows: src's table slots
    return bubble_on(err, dst, src, d, src->nbuckets * (uint64_t)src->S, dev_stats, (hipStream_t)sp);
}

int kc_pop_bubbles(kc_ctx* dst, kc_ctx* src, const kc_bubble_desc* d, kc_bubble_stats* stats) {
    kc_ctx* err = dst ? dst : src;
    if (!src || !d) return err ? err->fail(KC_ERR_ARG, "kc_pop_bubbles: null source or descriptor") : KC_ERR_ARG;
    int rc = bubble_check(err, dst, src, d);
    if (rc) return rc;
    DevBuf<kc_bubble_stats> ds;
    if (stats && !ds.reserve(1)) return err->fail(KC_ERR_NOMEM, "kc_pop_bubbles: statistics allocation failed");
    unsigned long long bound = 0;
    if ((rc = bubble_rc(err, src, unitig_bound(src, d->min_count, &bound)))) return rc;
    hipStream_t s = err->stream;
    rc = bubble_on(err, dst, src, d, bound, ds, s);
    hipError_t e = hipSuccess;
    if (rc == KC_OK && stats) e = hipMemcpyAsync(stats, ds, sizeof(kc_bubble_stats), hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);  // (also on an error: the kernels may still write ds)
    if (rc == KC_OK && (e != hipSuccess || e2 != hipSuccess))
        rc = err->hipfail(e != hipSuccess ? e : e2, "kc_pop_bubbles: statistics copy");
    return rc;
}

}  // extern "C"
