// kc_api_graph.cpp -- the de Bruijn graph of the counted table (include/kc_api.h kc_neighbors*,
// kc_graph*): the counts of the eight neighbours of given k-mers, and every node's edge bits,
// unitig-link bits and the whole graph's statistics.  Kernels: kc_graph_impl.h (k_neighbors; the
// sweep pair k_graph_edges / k_graph_links).
#include "kc_ctx.h"

#pragma GCC visibility push(hidden)

static_assert(sizeof(kc_graph_stats) == 80, "include/kc_api.h states this size");
static_assert(sizeof(kc_graph_stats) == (GRAPH_STAT_WORDS - 1) * sizeof(unsigned long long),
              "the statistics scratch: kc_graph_stats, then the record cursor");

// what every entry point checks before it touches the device
static int graph_ready(kc_ctx* c) {
    if (c->cfg.k < 2) return c->fail(KC_ERR_ARG, "the de Bruijn graph needs k >= 2");
    JOB_OK(c);
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table (kc_bloom_finalize must precede a graph query)");
    return KC_OK;
}

static int neighbors_check(kc_ctx* c, const uint64_t* keys, uint64_t n, int layout, const uint32_t* counts) {
    if (layout != KC_KEYS_DUMP && layout != KC_KEYS_TABLE) return c->fail(KC_ERR_ARG, "unknown key layout");
    if (n && (!keys || !counts)) return c->fail(KC_ERR_ARG, "null key or count array");
    return graph_ready(c);
}

static int graph_check(kc_ctx* c, uint32_t min_count, uint32_t max_count) {
    if (max_count && min_count > max_count) return c->fail(KC_ERR_ARG, "kc_graph: min_count is above max_count");
    return graph_ready(c);
}

#pragma GCC visibility pop

extern "C" {

int kc_neighbors_device(kc_ctx* c, const uint64_t* keys, uint64_t n, int layout, uint32_t* counts, void* sp) {
    if (!c) return KC_ERR_ARG;
    int rc = neighbors_check(c, keys, n, layout, counts);
    if (rc) return rc;
    if (n == 0) return KC_OK;
    hipStream_t s = (hipStream_t)sp;
    if ((rc = flush_host(c))) return rc;
    StreamScope on(c, s);
    if ((rc = on.join())) return rc;
    if ((rc = materialize_zero(c, s))) return rc;  // an emptied table answers 0
    HIPCHK(c, launch_neighbors(table_view(c), c->cfg.k, c->cfg.mode == 0 ? 0 : 1, layout, keys, n, counts, s));
    return on.finish();
}

int kc_neighbors(kc_ctx* c, const uint64_t* keys, uint64_t n, int layout, uint32_t* counts) {
    if (!c) return KC_ERR_ARG;
    int rc = neighbors_check(c, keys, n, layout, counts);
    if (rc) return rc;
    if (n == 0) return KC_OK;
    DevBuf<uint64_t> dk;
    DevBuf<uint32_t> dc;
    make_room(c, n * (c->W * 8 + 32));
    if (!dk.reserve(n * c->W) || !dc.reserve(n * 8)) return c->fail(KC_ERR_NOMEM, "neighbour buffers");
    hipError_t e = hipMemcpyAsync(dk, keys, n * c->W * 8, hipMemcpyHostToDevice, c->stream);
    rc = e == hipSuccess ? kc_neighbors_device(c, dk, n, layout, dc, c->stream) : c->hipfail(e, "neighbours: key copy");
    if (rc == KC_OK) {
        e = hipMemcpyAsync(counts, dc, n * 32, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = c->hipfail(e, "neighbours: count copy");
    } else {
        (void)hipStreamSynchronize(c->stream);  // (the key copy reads dk)
    }
    return rc;
}

int kc_graph_device(kc_ctx* c, uint32_t min_count, uint32_t max_count, uint64_t* records, uint64_t capacity,
                    uint64_t* n_records, kc_graph_stats* stats, void* sp) {
    if (!c) return KC_ERR_ARG;
    int rc = graph_check(c, min_count, max_count);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)sp;
    if ((rc = flush_host(c))) return rc;
    StreamScope on(c, s);
    if ((rc = on.join())) return rc;
    if ((rc = materialize_zero(c, s))) return rc;  // an emptied table has no nodes
    const uint64_t slots = c->nbuckets * (uint64_t)c->S;
    if (c->d_graph_edges.capacity() < slots) make_room(c, slots);
    if (!c->d_graph_edges.reserve(slots) || !c->d_graph_stat.reserve(GRAPH_STAT_WORDS))
        return c->fail(KC_ERR_NOMEM, "kc_graph: edge scratch allocation failed");
    unsigned long long* st = c->d_graph_stat;
    HIPCHK(c, hipMemsetAsync(st, 0, GRAPH_STAT_WORDS * sizeof(unsigned long long), s));
    HIPCHK(c, launch_graph(table_view(c), c->cfg.k, c->cfg.mode == 0 ? 0 : 1, min_count ? min_count : 1, max_count,
                           c->d_graph_edges, records, records ? capacity : 0, st, s));
    if (stats) HIPCHK(c, hipMemcpyAsync(stats, st, sizeof(kc_graph_stats), hipMemcpyDeviceToDevice, s));
    if (n_records) HIPCHK(c, hipMemcpyAsync(n_records, st, sizeof(uint64_t), hipMemcpyDeviceToDevice, s));  // nodes
    return on.finish();
}

int kc_graph(kc_ctx* c, uint32_t min_count, uint32_t max_count, uint64_t** records, uint64_t* n_records,
             kc_graph_stats* stats) {
    if (!c) return KC_ERR_ARG;
    if (records) *records = nullptr;
    if (n_records) *n_records = 0;
    int rc = graph_check(c, min_count, max_count);
    if (rc) return rc;
    const bool want = records && n_records;
    hipStream_t s = c->stream;
    const size_t rec = (size_t)(c->W + 1) * sizeof(uint64_t);
    // the records' capacity: the k-mers with T(c) >= min_count (one count-only sweep, as kc_dump's)
    unsigned long long cap = 0;
    if (want) {
        if ((rc = sync_for_read(c))) return rc;
        HIPCHK(c, hipMemsetAsync(&c->d_ctr->dump_n, 0, 16 * 8 * 2, s));  // dump_n + occupied lines
        HIPCHK(c, launch_dump(table_view(c), c->cfg.mode == 0 ? 0 : 1, min_count ? min_count : 1, nullptr, c->d_ctr, s));
        HIPCHK(c, hipMemcpyAsync(&cap, &c->d_ctr->dump_n, 8, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
    }
    DevBuf<uint64_t> d;
    DevBuf<unsigned long long> dst;  // kc_graph_stats
    DrainOnError drain{s};
    if (cap) make_room(c, cap * rec);
    if ((cap && !d.reserve(cap * (c->W + 1))) || !dst.reserve(GRAPH_STAT_WORDS - 1))
        return c->fail(KC_ERR_NOMEM, "kc_graph: record buffer allocation failed");
    kc_graph_stats h{};
    rc = kc_graph_device(c, min_count, max_count, cap ? d.get() : nullptr, cap, nullptr,
                         reinterpret_cast<kc_graph_stats*>(dst.get()), s);
    if (rc) return rc;
    HIPCHK(c, hipMemcpyAsync(&h, dst, sizeof(h), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (want) {
        const uint64_t n = std::min<uint64_t>(h.nodes, cap);
        HostRecords out((uint64_t*)std::malloc(std::max<size_t>(1, n * rec)));
        if (!out) return c->fail(KC_ERR_NOMEM, "host allocation failed");
        if (n) {
            HIPCHK(c, hipMemcpyAsync(out.get(), d, n * rec, hipMemcpyDeviceToHost, s));
            HIPCHK(c, hipStreamSynchronize(s));
        }
        *records = out.release();
        *n_records = n;
    }
    drain.done();
    if (stats) *stats = h;
    return KC_OK;
}

}  // extern "C"
