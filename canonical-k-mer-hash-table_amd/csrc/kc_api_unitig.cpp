// kc_api_unitig.cpp -- the unitigs of the counted table's de Bruijn graph (include/kc_api.h
// kc_unitigs*) and the compacted graph, the unitigs with the edges between them (kc_unitig_graph*):
// the checks, the scratch and the host forms.  Kernels: kc_unitig_impl.h (the sweeps that number the
// nodes and find the successor states, the bases, the edges) and kc_unitig.hip (the ranking, the
// cut of the circles, the records); the host arithmetic: kc_unitig_host.h.
#include "kc_ctx.h"

#pragma GCC visibility push(hidden)

static_assert(sizeof(kc_unitig) == 32 && sizeof(kc_unitig_stats) == 40, "include/kc_api.h states these sizes");
static_assert(sizeof(kc_unitig_stats) == 5 * sizeof(unsigned long long), "UC_STATS: five control words");
static_assert(sizeof(kc_unitig_edge) == 16 && sizeof(kc_cdbg_stats) == 64, "include/kc_api.h states these sizes");
static_assert(sizeof(kc_cdbg_stats) == (UC_CDBG_ZERO + 1 - UC_STATS) * sizeof(unsigned long long) && UC_CDBG_ZERO < UC_SRC &&
                  offsetof(kc_cdbg_stats, edges) == (UC_EDGES - UC_STATS) * 8 && offsetof(kc_cdbg_stats, dead_ends) == (UC_DEAD - UC_STATS) * 8,
              "kc_cdbg_stats is the control words from UC_STATS on");
static_assert(KC_EDGE_FROM_REV == 1 && KC_EDGE_TO_REV == 2, "k_unitig_edges writes from_rev | to_rev << 1");
static_assert(sizeof(UnitigState) * 4 + 4 + 8 + 8 + 4 + 4 + 16 == UNITIG_NODE_BYTES, "kc_unitig_host.h counts a node's bytes");

int unitig_check(kc_ctx* c, uint32_t min_count, uint32_t max_count) {
    if (c->cfg.k < 2) return c->fail(KC_ERR_ARG, "unitigs need k >= 2");
    if (max_count && min_count > max_count) return c->fail(KC_ERR_ARG, "kc_unitigs: min_count is above max_count");
    JOB_OK(c);
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table (kc_bloom_finalize must precede a unitig query)");
    return KC_OK;
}

static_assert(offsetof(kc_cdbg_stats, bases) == offsetof(kc_unitig_stats, bases) && offsetof(kc_cdbg_stats, max_nodes) == 4 * 8,
              "kc_unitig_stats is the first five words of kc_cdbg_stats");

// the views of c's scratch for `bound` node ids
static UnitigRanked unitig_bufs(const kc_ctx* c, uint64_t bound, UnitigWants w) {
    const UnitigLayout l = unitig_layout(bound, w);
    uint64_t* b = c->d_unitig_node;
    UnitigBufs u{};
    u.edges = c->d_graph_edges;
    u.id_of_slot = c->d_unitig_ids;
    u.bound = bound;
    u.st[0] = reinterpret_cast<UnitigState*>(b + l.st0);
    u.st[1] = reinterpret_cast<UnitigState*>(b + l.st1);
    u.slot_of = b + l.slot_of;
    u.off = b + l.off;
    u.succ = reinterpret_cast<uint32_t*>(b + l.succ);
    u.tc = reinterpret_cast<uint32_t*>(b + l.tc);
    u.start = reinterpret_cast<uint32_t*>(b + l.start);
    u.pos = reinterpret_cast<uint32_t*>(b + l.pos);
    u.ctl = c->d_unitig_ctl;
    u.verdict = w.verdict ? reinterpret_cast<uint8_t*>(b + l.verdict) : nullptr;
    return UnitigRanked{u, unitig_rounds(bound), w.anchors ? reinterpret_cast<uint32_t*>(b + l.anchors) : nullptr};
}

// The ranking on s for up to `bound` nodes (the caller has joined s): the scratch first -- a failure
// is reported before any kernel of the call is launched -- then the three sweeps and the jump
// launches.  Leaves the views and the rounds for unitig_write and for the filters' kernels
// (kc_api_filter.cpp).
int unitig_rank(kc_ctx* c, uint32_t min_count, uint32_t max_count, uint64_t bound, UnitigWants w, hipStream_t s,
                UnitigRanked* r) {
    const uint64_t slots = c->nbuckets * (uint64_t)c->S;
    bound = std::max<uint64_t>(1, std::min(bound, slots));
    if (bound >= UNITIG_MAX_BOUND)
        return c->fail(KC_ERR_NOMEM, "kc_unitigs: " + std::to_string(bound) + " node ids do not fit 32-bit states (the "
                                     "device form sizes by the table's slots, kc_unitigs by the k-mers from min_count on)");
    const uint64_t words = unitig_layout(bound, w).words;
    if (c->d_graph_edges.capacity() < slots || c->d_unitig_ids.capacity() < slots || c->d_unitig_node.capacity() < words ||
        (w.rec && c->d_unitig_rec.capacity() < bound))
        make_room(c, unitig_scratch_bytes(slots, bound, w));
    if (!c->d_graph_edges.reserve(slots) || !c->d_unitig_ids.reserve(slots) || !c->d_unitig_node.reserve(words) ||
        !c->d_unitig_ctl.reserve(UNITIG_CTL_WORDS) || (w.rec && !c->d_unitig_rec.reserve(bound)))
        return c->fail(KC_ERR_NOMEM, "kc_unitigs: scratch allocation failed (" +
                                     std::to_string(unitig_scratch_bytes(slots, bound, w)) + " bytes)");
    *r = unitig_bufs(c, bound, w);
    HIPCHK(c, hipMemsetAsync(r->u.ctl, 0, UNITIG_CTL_WORDS * sizeof(unsigned long long), s));
    HIPCHK(c, launch_unitig_succ(table_view(c), c->cfg.k, c->cfg.mode == 0 ? 0 : 1, min_count ? min_count : 1, max_count,
                                 r->u, s));
    HIPCHK(c, launch_unitig_rank(r->u, r->rounds, s));
    return KC_OK;
}

// the records and the bases of a ranking, each where its pointer is not NULL; rec
// (kc_unitig_graph*): the record indices this launch hands out, per start id
static int unitig_write(kc_ctx* c, const UnitigRanked& r, kc_unitig* recs, uint64_t cap_unitigs, uint8_t* bases,
                        uint64_t cap_bases, hipStream_t s, uint32_t* rec) {
    HIPCHK(c, launch_unitig_heads(r.u, c->cfg.k, r.rounds, recs, cap_unitigs, bases ? cap_bases : 0, rec, s));
    if (bases) HIPCHK(c, launch_unitig_emit(table_view(c), c->cfg.k, r.u, bases, s));
    return KC_OK;
}

// the ids' bound of the host forms: the k-mers with T(c) >= min_count (one count-only sweep, as
// kc_graph's); waits
int unitig_bound(kc_ctx* c, uint32_t min_count, unsigned long long* bound) {
    hipStream_t s = c->stream;
    int rc = sync_for_read(c);
    if (rc) return rc;
    HIPCHK(c, hipMemsetAsync(&c->d_ctr->dump_n, 0, 16 * 8 * 2, s));  // dump_n + occupied lines
    HIPCHK(c, launch_dump(table_view(c), c->cfg.mode == 0 ? 0 : 1, min_count ? min_count : 1, nullptr, c->d_ctr, s));
    HIPCHK(c, hipMemcpyAsync(bound, &c->d_ctr->dump_n, 8, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    return KC_OK;
}

// what a host form hands to its caller (who frees it with kc_free): n elements from dev, or an empty block
template <class T>
static int unitig_to_host(kc_ctx* c, std::unique_ptr<T, StdFree>* out, const T* dev, uint64_t n, hipStream_t s) {
    out->reset((T*)std::malloc(std::max<size_t>(1, n * sizeof(T))));
    if (!*out) return c->fail(KC_ERR_NOMEM, "host allocation failed");
    if (dev && n) HIPCHK(c, hipMemcpyAsync(out->get(), dev, n * sizeof(T), hipMemcpyDeviceToHost, s));
    return KC_OK;
}

// The device form of kc_unitigs* and, with_edges, of kc_unitig_graph*, which adds the record index
// per id to the scratch, the edges' launch and the three statistics words behind kc_unitig_stats.
// after (kc_read_paths_device, kc_api_path.cpp): its scratch before the ranking's, its kernels behind the call's.
int unitigs_device(kc_ctx* c, bool with_edges, uint32_t min_count, uint32_t max_count, kc_unitig* unitigs,
                   uint64_t cap_unitigs, uint8_t* bases, uint64_t cap_bases, kc_unitig_edge* edges, uint64_t cap_edges,
                   void* stats, hipStream_t s, UnitigAfter* after) {
    if (!c) return KC_ERR_ARG;
    int rc = unitig_check(c, min_count, max_count);
    if (rc) return rc;
    if (with_edges && ((uintptr_t)edges & 15))
        return c->fail(KC_ERR_ARG, "kc_unitig_graph_device: dev_edges is not 16-byte aligned");
    if ((rc = flush_host(c))) return rc;
    StreamScope on(c, s);
    if ((rc = on.join())) return rc;
    if ((rc = materialize_zero(c, s))) return rc;  // an emptied table has no unitigs
    if (after && (rc = after->prepare(c))) return rc;
    UnitigRanked r;
    // no host wait, so the ids are sized by what the host knows: the table's slots
    if ((rc = unitig_rank(c, min_count, max_count, c->nbuckets * (uint64_t)c->S, with_edges ? UNITIG_GRAPH : UNITIG_PLAIN, s, &r)))
        return rc;
    // the edges read the record numbering of this heads launch, the one whose records the caller receives
    uint32_t* rec = with_edges ? c->d_unitig_rec.get() : nullptr;
    if ((rc = unitig_write(c, r, unitigs, cap_unitigs, bases, cap_bases, s, rec))) return rc;
    if (with_edges) HIPCHK(c, launch_unitig_edges(table_view(c), c->cfg.k, r.u, rec, edges, cap_edges, s));
    if (stats)
        HIPCHK(c, hipMemcpyAsync(stats, r.u.ctl + UC_STATS, with_edges ? sizeof(kc_cdbg_stats) : sizeof(kc_unitig_stats),
                                 hipMemcpyDeviceToDevice, s));
    if (after && (rc = after->run(c, r, rec, s))) return rc;
    return on.finish();
}

// The host form of kc_unitigs* and, with_edges, of kc_unitig_graph*: rank once, read the totals
// (records and edges counted without buffers), allocate, write.
// after (kc_read_paths): behind the last records' launch, whose numbering rec holds; it waits itself.
int unitigs_host(kc_ctx* c, bool with_edges, uint32_t min_count, uint32_t max_count, kc_unitig** unitigs, uint8_t** bases,
                 kc_unitig_edge** edges, void* stats, UnitigAfter* after) {
    if (!c) return KC_ERR_ARG;
    if (unitigs) *unitigs = nullptr;
    if (bases) *bases = nullptr;
    if (edges) *edges = nullptr;
    int rc = unitig_check(c, min_count, max_count);
    if (rc) return rc;
    hipStream_t s = c->stream;
    unsigned long long bound = 0;
    if ((rc = unitig_bound(c, min_count, &bound))) return rc;
    UnitigRanked r;
    kc_cdbg_stats h{};  // (kc_unitigs: its first five words)
    const size_t stat_bytes = with_edges ? sizeof(kc_cdbg_stats) : sizeof(kc_unitig_stats);
    DevBuf<kc_unitig> dr;
    DevBuf<uint8_t> db;
    DevBuf<kc_unitig_edge> de;
    DrainOnError drain{s};
    if ((rc = unitig_rank(c, min_count, max_count, bound, with_edges ? UNITIG_GRAPH : UNITIG_PLAIN, s, &r))) return rc;
    uint32_t* rec = with_edges ? c->d_unitig_rec.get() : nullptr;
    if ((rc = unitig_write(c, r, nullptr, 0, nullptr, 0, s, rec))) return rc;
    if (with_edges) HIPCHK(c, launch_unitig_edges(table_view(c), c->cfg.k, r.u, rec, nullptr, 0, s));
    HIPCHK(c, hipMemcpyAsync(&h, r.u.ctl + UC_STATS, stat_bytes, hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    const bool want_r = unitigs && h.unitigs, want_b = bases && h.bases, want_e = edges && h.edges;
    if (want_r || want_b || want_e) {
        make_room(c, h.unitigs * sizeof(kc_unitig) + h.bases + h.edges * sizeof(kc_unitig_edge));
        if ((want_r && !dr.reserve(h.unitigs)) || (want_b && !db.reserve(h.bases)) || (want_e && !de.reserve(h.edges)))
            return c->fail(KC_ERR_NOMEM, with_edges ? "kc_unitig_graph: record, base and edge buffer allocation failed"
                                                    : "kc_unitigs: record and base buffer allocation failed");
        // the records' launch numbers them anew, and the edges after it read that numbering
        if ((rc = unitig_write(c, r, want_r ? dr.get() : nullptr, h.unitigs, want_b ? db.get() : nullptr, h.bases, s, rec)))
            return rc;
        if (want_e) HIPCHK(c, launch_unitig_edges(table_view(c), c->cfg.k, r.u, rec, de.get(), h.edges, s));
    }
    if (after && (rc = after->run(c, r, rec, s))) return rc;
    std::unique_ptr<kc_unitig, StdFree> out_r;
    std::unique_ptr<uint8_t, StdFree> out_b;
    std::unique_ptr<kc_unitig_edge, StdFree> out_e;
    if (unitigs && (rc = unitig_to_host(c, &out_r, want_r ? dr.get() : nullptr, h.unitigs, s))) return rc;
    if (bases && (rc = unitig_to_host(c, &out_b, want_b ? db.get() : nullptr, h.bases, s))) return rc;
    if (edges && (rc = unitig_to_host(c, &out_e, want_e ? de.get() : nullptr, h.edges, s))) return rc;
    HIPCHK(c, hipStreamSynchronize(s));
    drain.done();
    if (unitigs) *unitigs = out_r.release();
    if (bases) *bases = out_b.release();
    if (edges) *edges = out_e.release();
    if (stats) std::memcpy(stats, &h, stat_bytes);
    return KC_OK;
}

#pragma GCC visibility pop

extern "C" {

int kc_unitigs_device(kc_ctx* c, uint32_t min_count, uint32_t max_count, kc_unitig* unitigs, uint64_t cap_unitigs,
                      uint8_t* bases, uint64_t cap_bases, kc_unitig_stats* stats, void* sp) {
    return unitigs_device(c, false, min_count, max_count, unitigs, cap_unitigs, bases, cap_bases, nullptr, 0, stats,
                          (hipStream_t)sp, nullptr);
}

int kc_unitigs(kc_ctx* c, uint32_t min_count, uint32_t max_count, kc_unitig** unitigs, uint8_t** bases,
               kc_unitig_stats* stats) {
    return unitigs_host(c, false, min_count, max_count, unitigs, bases, nullptr, stats, nullptr);
}

// ---- the compacted graph: the unitigs and the edges between them (kc_unitig_graph*) -----------------
int kc_unitig_graph_device(kc_ctx* c, uint32_t min_count, uint32_t max_count, kc_unitig* unitigs, uint64_t cap_unitigs,
                           uint8_t* bases, uint64_t cap_bases, kc_unitig_edge* edges, uint64_t cap_edges,
                           kc_cdbg_stats* stats, void* sp) {
    return unitigs_device(c, true, min_count, max_count, unitigs, cap_unitigs, bases, cap_bases, edges, cap_edges, stats,
                          (hipStream_t)sp, nullptr);
}

int kc_unitig_graph(kc_ctx* c, uint32_t min_count, uint32_t max_count, kc_unitig** unitigs, uint8_t** bases,
                    kc_unitig_edge** edges, kc_cdbg_stats* stats) {
    return unitigs_host(c, true, min_count, max_count, unitigs, bases, edges, stats, nullptr);
}

}  // extern "C"
