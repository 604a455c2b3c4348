// kc_api_filter.cpp -- the graph filters (include/kc_api.h): graph cleaning (kc_clean*), the graph of
// src's range without its short tips and short isolated unitigs, bubble popping (kc_pop_bubbles*),
// that graph without the weaker of its parallel unitigs, and weak-link removal (kc_cut_weak*), that
// graph without its short interior unitigs of low local coverage, each added into dst as a counted
// table.  They are one call: the ranking of kc_unitigs* (kc_api_unitig.cpp unitig_rank, on
// src's scratch, with one verdict byte per id on top), the filter's own verdict kernels, and the copy
// of the kept nodes k_clean (kc_clean_impl.h).  A Filter below says what differs.  The verdict
// kernels: k_unitig_verdict (kc_unitig.hip); k_bubble_anchors and k_bubble_verdict
// (kc_bubble_impl.h), which want two anchors per id in the scratch too; k_weak_verdict
// (kc_weak_impl.h).
#include <functional>

#include "kc_ctx.h"

#pragma GCC visibility push(hidden)

static_assert(sizeof(kc_clean_desc) == 24 && sizeof(kc_clean_stats) == 64, "include/kc_api.h states these sizes");
static_assert(sizeof(kc_clean_stats) == 8 * sizeof(unsigned long long) && offsetof(kc_clean_stats, tips) == 2 * 8 &&
                  offsetof(kc_clean_stats, isolated) == 4 * 8 && offsetof(kc_clean_stats, out_keys) == 6 * 8,
              "k_unitig_verdict adds words 0-5, k_clean words 6 and 7");
static_assert(UNITIG_NODE_BYTES + UNITIG_VERDICT_BYTES == 141, "include/kc_api.h states the scratch of kc_clean*");
static_assert(sizeof(kc_bubble_desc) == 24 && sizeof(kc_bubble_stats) == 64, "include/kc_api.h states these sizes");
static_assert(sizeof(kc_bubble_stats) == 8 * sizeof(unsigned long long) && offsetof(kc_bubble_stats, branches) == 2 * 8 &&
                  offsetof(kc_bubble_stats, parallel) == 3 * 8 && offsetof(kc_bubble_stats, out_keys) == 6 * 8,
              "k_bubble_anchors adds words 0-2, k_bubble_verdict words 3-5, k_clean words 6 and 7");
static_assert(UNITIG_NODE_BYTES + UNITIG_VERDICT_BYTES + UNITIG_ANCHOR_BYTES == 149,
              "include/kc_api.h states the scratch of kc_pop_bubbles*");
static_assert(sizeof(kc_weak_desc) == 24 && sizeof(kc_weak_stats) == 64, "include/kc_api.h states these sizes");
static_assert(sizeof(kc_weak_stats) == 8 * sizeof(unsigned long long) && offsetof(kc_weak_stats, interior) == 2 * 8 &&
                  offsetof(kc_weak_stats, cut) == 4 * 8 && offsetof(kc_weak_stats, out_keys) == 6 * 8,
              "k_weak_verdict adds words 0-5, k_clean words 6 and 7");

// the statistics of every filter (the assertions above): the verdict kernels add words 0-5, k_clean
// out_keys and out_sum at 6 and 7
struct FilterStats {
    unsigned long long w[8];
};

// What tells one filter from the others: its words in the messages, the fields all descriptors
// carry, what is wrong with its own fields (nullptr: nothing), what its ranking wants in the
// scratch, and the launch of its verdict kernels on the ranked graph of src (after
// launch_unitig_heads, before launch_clean).
struct Filter {
    const char* name;  // "kc_clean"
    const char* noun;  // "a graph cleaning"
    uint32_t min_count, max_count, reserved;
    const char* bad;   // ": ratio_permille must be at most 1000"
    UnitigWants wants;
    std::function<hipError_t(kc_ctx* src, const UnitigRanked& r, unsigned long long* stats, hipStream_t s)> verdict;
};

static Filter clean_filter(const kc_clean_desc* d) {
    const CleanRule rule{d->tip_max_nodes, d->iso_max_nodes, d->max_mean};
    return {"kc_clean", "a graph cleaning", d->min_count, d->max_count, d->reserved, nullptr, UNITIG_CLEAN,
            [rule](kc_ctx* src, const UnitigRanked& r, unsigned long long* stats, hipStream_t s) {
                return launch_unitig_verdict(r.u, r.rounds, src->nbuckets * (uint64_t)src->S, rule, stats, s);
            }};
}

// W-dispatch of the two kernels (kc_bubble_w.hip, one translation unit per key width)
static hipError_t launch_bubble(TableView src, int k, UnitigBufs u, int rounds, uint32_t* anc, BubbleRule rule,
                                unsigned long long* stats, hipStream_t s) {
    KC_DISPATCH(BubbleOps, src.W, pop(src, k, u, rounds, anc, rule, stats, s));
}

static Filter bubble_filter(const kc_bubble_desc* d) {
    const BubbleRule rule{d->max_nodes, d->max_diff, d->max_mean};
    return {"kc_pop_bubbles", "a bubble popping", d->min_count, d->max_count, d->reserved, nullptr, UNITIG_BUBBLE,
            [rule](kc_ctx* src, const UnitigRanked& r, unsigned long long* stats, hipStream_t s) {
                return launch_bubble(table_view(src), src->cfg.k, r.u, r.rounds, r.anchors, rule, stats, s);
            }};
}

// W-dispatch of the kernel (kc_weak_w.hip, one translation unit per key width)
static hipError_t launch_weak(TableView src, int k, UnitigBufs u, int rounds, WeakRule rule, unsigned long long* stats,
                              hipStream_t s) {
    KC_DISPATCH(WeakOps, src.W, cut(src, k, u, rounds, rule, stats, s));
}

static Filter weak_filter(const kc_weak_desc* d) {
    const WeakRule rule{d->max_nodes, d->ratio_permille, d->max_mean};
    const char* bad = d->ratio_permille > 1000 ? ": ratio_permille must be at most 1000"
                      : d->max_nodes && !d->ratio_permille && !d->max_mean
                          ? ": max_nodes needs ratio_permille or max_mean (every short interior unitig would be cut)"
                          : nullptr;
    return {"kc_cut_weak", "a weak-link removal", d->min_count, d->max_count, d->reserved, bad, UNITIG_CLEAN,
            [rule](kc_ctx* src, const UnitigRanked& r, unsigned long long* stats, hipStream_t s) {
                return launch_weak(table_view(src), src->cfg.k, r.u, r.rounds, rule, stats, s);
            }};
}

// what both forms check before they touch the device; err receives the message
static int filter_check(const Filter& f, kc_ctx* err, kc_ctx* dst, kc_ctx* src) {
    const std::string name = f.name;
    if (dst == src) return err->fail(KC_ERR_ARG, name + ": dst must not be src");
    if (dst && (dst->cfg.k != src->cfg.k || dst->cfg.device != src->cfg.device))
        return err->fail(KC_ERR_ARG, name + ": the contexts must have the same k and device");
    if (f.reserved) return err->fail(KC_ERR_ARG, name + ": reserved must be 0");
    if (f.bad) return err->fail(KC_ERR_ARG, name + f.bad);
    // k < 2, min_count above a non-zero max_count; then src's job and table
    int rc = route_rc(err, src, unitig_check(src, f.min_count, f.max_count));
    if (rc) return rc;
    if (dst) {
        if (!dst->broken.empty()) return err->fail(KC_ERR_STATE, dst->broken + " (kc_reset first)");
        if (!dst->nbuckets)
            return err->fail(KC_ERR_STATE, std::string("no table (kc_bloom_finalize must precede ") + f.noun + ")");
    }
    return KC_OK;
}

// The call on s with `bound` node ids (the caller has checked).  No host wait.
static int filter_on(const Filter& f, kc_ctx* err, kc_ctx* dst, kc_ctx* src, uint64_t bound, FilterStats* dev_stats,
                     hipStream_t s) {
    int rc;
    for (kc_ctx* x : {dst, src})
        if (x && (rc = route_rc(err, x, flush_host(x)))) return rc;
    StreamScope on_s(src, s);
    if ((rc = route_rc(err, src, on_s.join()))) return rc;
    // an emptied src has no unitigs (and its memory is not read before it is zeroed)
    if ((rc = route_rc(err, src, materialize_zero(src, s)))) return rc;
    UnitigRanked r;
    // the scratch first: KC_ERR_NOMEM before any kernel of the call
    if ((rc = route_rc(err, src, unitig_rank(src, f.min_count, f.max_count, bound, f.wants, s, &r)))) return rc;
    unsigned long long* st = dev_stats ? dev_stats->w : nullptr;
    if (st) HIPCHK(err, hipMemsetAsync(st, 0, sizeof(FilterStats), s));
    const TableView ts = table_view(src);
    HIPCHK(err, launch_unitig_heads(r.u, src->cfg.k, r.rounds, nullptr, 0, 0, nullptr, s));
    HIPCHK(err, f.verdict(src, r, st, s));
    rc = write_dst(dst, s, [&]() -> int {
        HIPCHK(err, launch_clean(ts, dst ? table_view(dst) : TableView{}, r.u, dst ? dst->d_ctr.get() : nullptr, st, s));
        return KC_OK;
    });
    if (rc) return rc;
    return route_rc(err, src, on_s.finish());
}

// the device form (stream given) and the host form (stats to host memory, waits) of a filter
static int filter_device(const Filter& f, kc_ctx* dst, kc_ctx* src, void* dev_stats, void* sp) {
    kc_ctx* err = dst ? dst : src;
    int rc = filter_check(f, err, dst, src);
    if (rc) return rc;
    // no host wait, so the ids are sized by what the host knows: src's table slots
    return filter_on(f, err, dst, src, src->nbuckets * (uint64_t)src->S, (FilterStats*)dev_stats, (hipStream_t)sp);
}

static int filter_host(const Filter& f, kc_ctx* dst, kc_ctx* src, void* stats) {
    kc_ctx* err = dst ? dst : src;
    int rc = filter_check(f, err, dst, src);
    if (rc) return rc;
    return stats_host_form(err, f.name, (FilterStats*)stats, [&](FilterStats* ds, hipStream_t s) {
        unsigned long long bound = 0;
        const int rb = route_rc(err, src, unitig_bound(src, f.min_count, &bound));
        return rb ? rb : filter_on(f, err, dst, src, bound, ds, s);
    });
}

static int filter_null(kc_ctx* err, const char* name) {
    return err ? err->fail(KC_ERR_ARG, std::string(name) + ": null source or descriptor") : KC_ERR_ARG;
}

#pragma GCC visibility pop

extern "C" {

int kc_clean_device(kc_ctx* dst, kc_ctx* src, const kc_clean_desc* d, kc_clean_stats* dev_stats, void* sp) {
    if (!src || !d) return filter_null(dst ? dst : src, "kc_clean");
    return filter_device(clean_filter(d), dst, src, dev_stats, sp);
}

int kc_clean(kc_ctx* dst, kc_ctx* src, const kc_clean_desc* d, kc_clean_stats* stats) {
    if (!src || !d) return filter_null(dst ? dst : src, "kc_clean");
    return filter_host(clean_filter(d), dst, src, stats);
}

int kc_pop_bubbles_device(kc_ctx* dst, kc_ctx* src, const kc_bubble_desc* d, kc_bubble_stats* dev_stats, void* sp) {
    if (!src || !d) return filter_null(dst ? dst : src, "kc_pop_bubbles");
    return filter_device(bubble_filter(d), dst, src, dev_stats, sp);
}

int kc_pop_bubbles(kc_ctx* dst, kc_ctx* src, const kc_bubble_desc* d, kc_bubble_stats* stats) {
    if (!src || !d) return filter_null(dst ? dst : src, "kc_pop_bubbles");
    return filter_host(bubble_filter(d), dst, src, stats);
}

int kc_cut_weak_device(kc_ctx* dst, kc_ctx* src, const kc_weak_desc* d, kc_weak_stats* dev_stats, void* sp) {
    if (!src || !d) return filter_null(dst ? dst : src, "kc_cut_weak");
    return filter_device(weak_filter(d), dst, src, dev_stats, sp);
}

int kc_cut_weak(kc_ctx* dst, kc_ctx* src, const kc_weak_desc* d, kc_weak_stats* stats) {
    if (!src || !d) return filter_null(dst ? dst : src, "kc_cut_weak");
    return filter_host(weak_filter(d), dst, src, stats);
}

}  // extern "C"
