// kc_api_read.cpp -- the readers of the counted table: dump, output digest, the compact
// representation, key lookups, the abundance histogram and the text writer (include/kc_api.h).
#include "kc_ctx.h"

extern "C" {

int kc_dump(kc_ctx* c, uint64_t** records, uint64_t* n_records) {
    if (!c || !records || !n_records) return KC_ERR_ARG;
    *records = nullptr;
    *n_records = 0;
    int rc = sync_for_read(c);
    if (rc) return rc;
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table");
    TableView tv = table_view(c);
    const int cm = c->cfg.mode == 0 ? 0 : 1;
    const uint64_t a = c->cfg.min_abundance;
    HIPCHK(c, hipMemsetAsync(&c->d_ctr->dump_n, 0, 16 * 8 * 2, c->stream));  // dump_n + occupied lines
    HIPCHK(c, launch_dump(tv, cm, a, nullptr, c->d_ctr, c->stream));
    unsigned long long n = 0;
    HIPCHK(c, hipMemcpyAsync(&n, &c->d_ctr->dump_n, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t rec = (size_t)(c->W + 1) * sizeof(uint64_t);
    HostRecords h((uint64_t*)std::malloc(std::max<size_t>(1, n * rec)));
    if (!h) return c->fail(KC_ERR_NOMEM, "host allocation failed");
    if (n) {
        DevBuf<uint64_t> d;
        DrainOnError drain{c->stream};
        make_room(c, n * rec);
        if (!d.reserve(n * (c->W + 1))) return c->fail(KC_ERR_NOMEM, "dump buffer allocation failed");
        HIPCHK(c, hipMemsetAsync(&c->d_ctr->dump_n, 0, 16 * 8 * 2, c->stream));
        HIPCHK(c, launch_dump(tv, cm, a, d, c->d_ctr, c->stream));
        HIPCHK(c, hipMemcpyAsync(h.get(), d, n * rec, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        drain.done();
    }
    *records = h.release();
    *n_records = n;
    return KC_OK;
}

int kc_output_digest(kc_ctx* c, kc_digest* out) {
    if (!c || !out) return KC_ERR_ARG;
    std::memset(out, 0, sizeof(*out));
    if (c->cfg.min_abundance == 0) return KC_OK;  // no output (parallel_parser.hpp:1536 / 858)
    int rc = sync_for_read(c);
    if (rc) return rc;
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table");
    DevBuf<unsigned long long> d;
    if (!d.reserve(4)) return c->fail(KC_ERR_NOMEM, "digest buffer allocation failed");
    unsigned long long h[4] = {0, 0, 0, 0};
    hipError_t e = hipMemsetAsync(d, 0, sizeof(h), c->stream);
    if (e == hipSuccess)
        e = launch_text_digest(table_view(c), c->cfg.mode == 0 ? 0 : 1, c->cfg.min_abundance, c->cfg.k, d, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);  // (the kernel may still write d)
        return c->fail(KC_ERR_HIP, std::string("output digest: ") + hipGetErrorString(e));
    }
    out->lines = h[0];
    out->count_sum = h[1];
    out->hash_sum = h[2];
    out->hash_xor = h[3];
    return KC_OK;
}

// ------------------------------------------------------------------------------
// Kaarme's compact representation: kc_compact_impl.h
// ------------------------------------------------------------------------------
int kc_compact(kc_ctx* c, double load, kc_compact_info* info) {
    if (!c) return KC_ERR_ARG;
    if (load == 0) load = 0.8;
    if (!(load > 0 && load <= 0.95)) return c->fail(KC_ERR_ARG, "load must be in (0, 0.95]");
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table");
    if (c->cfg.mode == 0)
        return c->fail(KC_ERR_UNSUPPORTED, "the compact representation holds Kaarme counts (-m 1/2: 14 bits, "
                                           "saturating at 16383)");
    int rc = sync_for_read(c);
    if (rc) return rc;
    rc = materialize_zero(c, c->stream);
    if (rc) return rc;
    drop_compact(c);
    const TableView tv = table_view(c);
    HIPCHK(c, hipMemsetAsync(&c->d_ctr->occupied, 0, 8, c->stream));
    HIPCHK(c, launch_dump(tv, 1, ~0ULL, nullptr, c->d_ctr, c->stream));
    unsigned long long occ = 0;
    HIPCHK(c, hipMemcpyAsync(&occ, &c->d_ctr->occupied, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t nslots = std::max<uint64_t>(64, (uint64_t)std::ceil((double)occ / load));
    if (nslots >> 38) return c->fail(KC_ERR_ARG, "too many k-mers for 38-bit slot pointers");
    DevBuf<uint64_t> src, second, inv;
    DrainOnError drain{c->stream};
    if (!c->d_cstat.reserve(4)) return c->fail(KC_ERR_NOMEM, "compact counters");
    make_room(c, nslots * 16 + std::max<uint64_t>(1, occ) * c->W * 8 + c->nbuckets * c->S * 8);
    if (!c->d_cwords.reserve(nslots) || !src.reserve(nslots) || !second.reserve(std::max<uint64_t>(1, occ) * c->W) ||
        !inv.reserve(c->nbuckets * c->S)) {
        drop_compact(c);
        return c->fail(KC_ERR_NOMEM, "compact representation allocation failed");
    }
    HIPCHK(c, hipMemsetAsync(c->d_cwords, 0, nslots * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(src, 0xFF, nslots * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_cstat, 0, 4 * sizeof(unsigned long long), c->stream));
    CompactView cv{c->d_cwords, nslots, src, second, c->d_cstat, inv};
    HIPCHK(c, launch_compact_build(tv, cv, c->cfg.k, c->stream));
    unsigned long long starts = 0;
    HIPCHK(c, hipMemcpyAsync(&starts, c->d_cstat, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    reset_all(src, inv);
    // the secondary array at its size (the reference grows it as chains start, :2267-2278)
    if (!c->d_csecond.reserve(std::max<uint64_t>(1, starts) * c->W)) {
        drop_compact(c);
        return c->fail(KC_ERR_NOMEM, "secondary array allocation failed");
    }
    if (starts) HIPCHK(c, hipMemcpyAsync(c->d_csecond, second, starts * c->W * 8, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    drain.done();
    second.reset();
    c->cslots = nslots;
    c->cstarts = starts;
    c->ckmers = occ;
    if (info) {
        info->slots = nslots;
        info->kmers = occ;
        info->chain_starts = starts;
        info->bytes = nslots * 8 + starts * c->W * 8;
        info->table_bytes = c->nbuckets * BUCKET_WORDS * 8;
    }
    return KC_OK;
}

static CompactView compact_view(const kc_ctx* c) {
    return CompactView{c->d_cwords, c->cslots, nullptr, c->d_csecond, c->d_cstat};
}

int kc_compact_dump(kc_ctx* c, uint64_t** records, uint64_t* n_records, uint64_t* max_hops, double* mean_hops) {
    if (!c || !records || !n_records) return KC_ERR_ARG;
    *records = nullptr;
    *n_records = 0;
    if (!c->d_cwords) return c->fail(KC_ERR_STATE, "no compact representation (kc_compact)");
    int rc = sync_for_read(c);
    if (rc) return rc;
    const CompactView cv = compact_view(c);
    const uint64_t a = c->cfg.min_abundance;
    unsigned long long st[4];
    HIPCHK(c, hipMemsetAsync(c->d_cstat, 0, sizeof(st), c->stream));
    HIPCHK(c, launch_compact_dump(c->W, cv, c->cfg.k, a, nullptr, c->d_cstat, c->d_cstat + 1, c->stream));
    HIPCHK(c, hipMemcpyAsync(st, c->d_cstat, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t n = st[0];
    if (st[3]) return c->fail(KC_ERR_STATE, std::to_string(st[3]) + " compact slots did not reconstruct");
    const size_t rec = (size_t)(c->W + 1) * sizeof(uint64_t);
    HostRecords h((uint64_t*)std::malloc(std::max<size_t>(1, n * rec)));
    if (!h) return c->fail(KC_ERR_NOMEM, "host allocation failed");
    if (n) {
        DevBuf<uint64_t> d;
        DrainOnError drain{c->stream};
        make_room(c, n * rec);
        if (!d.reserve(n * (c->W + 1))) return c->fail(KC_ERR_NOMEM, "dump buffer allocation failed");
        HIPCHK(c, hipMemsetAsync(c->d_cstat, 0, sizeof(st), c->stream));
        HIPCHK(c, launch_compact_dump(c->W, cv, c->cfg.k, a, d, c->d_cstat, c->d_cstat + 1, c->stream));
        HIPCHK(c, hipMemcpyAsync(h.get(), d, n * rec, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(st, c->d_cstat, sizeof(st), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        drain.done();
    }
    if (max_hops) *max_hops = st[2];
    if (mean_hops) *mean_hops = n ? (double)st[1] / (double)n : 0.0;
    *records = h.release();
    *n_records = n;
    return KC_OK;
}

int kc_compact_lookup(kc_ctx* c, const uint64_t* keys, uint64_t n, uint32_t* counts) {
    if (!c || (n && (!keys || !counts))) return KC_ERR_ARG;
    if (!c->d_cwords) return c->fail(KC_ERR_STATE, "no compact representation (kc_compact)");
    if (!n) return KC_OK;
    int rc = sync_for_read(c);
    if (rc) return rc;
    DevBuf<uint64_t> dk;
    DevBuf<uint32_t> dc;
    DrainOnError drain{c->stream};
    if (!dk.reserve(n * c->W) || !dc.reserve(n)) return c->fail(KC_ERR_NOMEM, "lookup buffers");
    HIPCHK(c, hipMemcpyAsync(dk, keys, n * c->W * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, launch_compact_lookup(c->W, compact_view(c), c->cfg.k, dk, n, dc, c->stream));
    HIPCHK(c, hipMemcpyAsync(counts, dc, n * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    drain.done();
    return KC_OK;
}

// ------------------------------------------------------------------------------
// Queries of the counted full-key table: kc_query_impl.h (the reference has none: its table
// is only walked by the writers, kmer_hash_table.cpp:4318-4524)
// ------------------------------------------------------------------------------
int kc_lookup_device(kc_ctx* c, const uint64_t* keys, uint64_t n, int layout, uint32_t* counts, void* sp) {
    if (!c) return KC_ERR_ARG;
    if (layout != KC_KEYS_DUMP && layout != KC_KEYS_TABLE) return c->fail(KC_ERR_ARG, "unknown key layout");
    if (n && (!keys || !counts)) return c->fail(KC_ERR_ARG, "null key or count array");
    JOB_OK(c);
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table (kc_bloom_finalize must precede a lookup)");
    if (n == 0) return KC_OK;
    hipStream_t s = (hipStream_t)sp;
    int rc = flush_host(c);
    if (rc) return rc;
    StreamScope on(c, s);
    if ((rc = on.join())) return rc;
    rc = materialize_zero(c, s);  // an emptied table answers 0
    if (rc) return rc;
    HIPCHK(c, launch_lookup(table_view(c), c->cfg.k, c->cfg.mode == 0 ? 0 : 1, layout, keys, n, counts, s));
    return on.finish();  // the context's later work (counting into the table) follows the lookup
}

int kc_lookup(kc_ctx* c, const uint64_t* keys, uint64_t n, int layout, uint32_t* counts) {
    if (!c) return KC_ERR_ARG;
    if (layout != KC_KEYS_DUMP && layout != KC_KEYS_TABLE) return c->fail(KC_ERR_ARG, "unknown key layout");
    if (n && (!keys || !counts)) return c->fail(KC_ERR_ARG, "null key or count array");
    JOB_OK(c);
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table (kc_bloom_finalize must precede a lookup)");
    if (n == 0) return KC_OK;
    DevBuf<uint64_t> dk;
    DevBuf<uint32_t> dc;
    make_room(c, n * (c->W * 8 + 4));
    if (!dk.reserve(n * c->W) || !dc.reserve(n)) return c->fail(KC_ERR_NOMEM, "lookup buffers");
    hipError_t e = hipMemcpyAsync(dk, keys, n * c->W * 8, hipMemcpyHostToDevice, c->stream);
    int rc = e == hipSuccess ? kc_lookup_device(c, dk, n, layout, dc, c->stream) : c->hipfail(e, "lookup: key copy");
    if (rc == KC_OK) {
        e = hipMemcpyAsync(counts, dc, n * 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = c->hipfail(e, "lookup: count copy");
    } else {
        (void)hipStreamSynchronize(c->stream);  // (the key copy reads dk)
    }
    return rc;
}

int kc_histogram(kc_ctx* c, uint64_t* hist, uint32_t n_bins) {
    if (!c) return KC_ERR_ARG;
    if (!hist || n_bins < 2 || n_bins > 65537) return c->fail(KC_ERR_ARG, "kc_histogram: 2 <= n_bins <= 65537");
    int rc = sync_for_read(c);
    if (rc) return rc;
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table");
    DevBuf<unsigned long long> d;
    const size_t bytes = (size_t)n_bins * sizeof(unsigned long long);
    if (!d.reserve(n_bins)) return c->fail(KC_ERR_NOMEM, "histogram buffer allocation failed");
    hipError_t e = hipMemsetAsync(d, 0, bytes, c->stream);
    if (e == hipSuccess) e = launch_histo(table_view(c), c->cfg.mode == 0 ? 0 : 1, n_bins, d, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(hist, d, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);  // (the kernel may still write d)
        return c->fail(KC_ERR_HIP, std::string("histogram: ") + hipGetErrorString(e));
    }
    return KC_OK;
}

int kc_compact_read(kc_ctx* c, uint64_t* words, uint64_t n_words, uint64_t* second, uint64_t n_second_words) {
    if (!c) return KC_ERR_ARG;
    if (!c->d_cwords) return c->fail(KC_ERR_STATE, "no compact representation (kc_compact)");
    if (n_words > c->cslots || n_second_words > c->cstarts * c->W || (n_words && !words) ||
        (n_second_words && !second))
        return c->fail(KC_ERR_ARG, "more words than the compact representation holds");
    int rc = sync_for_read(c);
    if (rc) return rc;
    if (n_words) HIPCHK(c, hipMemcpy(words, c->d_cwords, n_words * 8, hipMemcpyDeviceToHost));
    if (n_second_words) HIPCHK(c, hipMemcpy(second, c->d_csecond, n_second_words * 8, hipMemcpyDeviceToHost));
    return KC_OK;
}

// Text output formatted on the device (the reference formats on one host
// thread, kmer_hash_table.cpp:4318-4524): k_text_bytes + scan give every TEXT_T-bucket
// block its offset in the text, then pieces of <= KC_TEXT_PIECE bytes are formatted by
// k_text, copied to pinned memory and written while the next piece is formatted
// (64 MiB pieces; KC_TEXT_PIECE overrides, >= 128 KiB so a block always fits).
// Lines come out in table order (the reference's order is unspecified too).
static uint64_t text_piece_bytes() {
    const char* e = std::getenv("KC_TEXT_PIECE");  // tests: force many pieces
    const uint64_t v = e ? std::strtoull(e, nullptr, 10) : 0;
    return v ? std::max<uint64_t>(v, 1ull << 17) : 64ull << 20;
}

int kc_write(kc_ctx* c, const char* path) {
    if (!c || !path) return KC_ERR_ARG;
    if (c->cfg.min_abundance == 0) return KC_OK;  // parallel_parser.hpp:1536 / 858
    int rc = sync_for_read(c);
    if (rc) return rc;
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table");
    const TableView tv = table_view(c);
    const int cm = c->cfg.mode == 0 ? 0 : 1;
    const uint64_t a = c->cfg.min_abundance;
    const uint64_t nblk = (c->nbuckets + TEXT_T - 1) / TEXT_T;
    DevBuf<uint32_t> d_bb;
    DevBuf<uint64_t> d_off, d_bsum;
    DevBuf<uint8_t> d_txt[2];
    PinnedBuf<uint8_t> h_txt[2];
    struct Events {
        hipEvent_t e[2] = {nullptr, nullptr};
        ~Events() {
            for (auto x : e)
                if (x) hipEventDestroy(x);
        }
    } events;
    auto& ev = events.e;
    std::vector<uint64_t> off(nblk + 1);
    std::vector<uint32_t> bb(nblk);
    std::unique_ptr<FILE, int (*)(FILE*)> file(nullptr, &std::fclose);
    // every return, the last one too, waits for the stream before the buffers above are freed
    DrainOnError drain{c->stream};
    if (!d_bb.reserve(nblk) || !d_off.reserve(nblk + 1) || !d_bsum.reserve((nblk + 4095) / 4096 + 2))
        return c->fail(KC_ERR_NOMEM, "text offset allocation failed");
    HIPCHK(c, launch_text_bytes(tv, cm, a, c->cfg.k, d_bb, d_off, d_bsum, c->stream));
    HIPCHK(c, hipMemcpyAsync(off.data(), d_off, (nblk + 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(bb.data(), d_bb, nblk * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const uint64_t total = off[nblk];
    file.reset(std::fopen(path, "wb"));
    FILE* f = file.get();
    if (!f) return c->fail(KC_ERR_IO, std::string("cannot open ") + path);
    // pieces: maximal runs of blocks whose text fits one piece buffer (a block's text is
    // at most TEXT_T * S * (k + 7) bytes < 128 KiB, so every block fits)
    const uint64_t cap = std::min<uint64_t>(text_piece_bytes(), std::max<uint64_t>(total, 1));
    struct Piece { uint64_t b0, b1; uint32_t lds; };
    std::vector<Piece> pieces;
    for (uint64_t b0 = 0; b0 < nblk;) {
        uint64_t b1 = b0;
        uint32_t mx = 0;
        while (b1 < nblk && off[b1 + 1] - off[b0] <= cap) mx = std::max(mx, bb[b1++]);
        if (b1 == b0) return c->fail(KC_ERR_STATE, "text block larger than a piece");
        if (off[b1] > off[b0]) pieces.push_back({b0, b1, (mx + 15) & ~15u});
        b0 = b1;
    }
    const int nbuf = pieces.size() > 1 ? 2 : 1;
    for (int i = 0; i < nbuf && !pieces.empty(); i++) {
        if (!d_txt[i].reserve(cap) || !h_txt[i].reserve(cap))
            return c->fail(KC_ERR_NOMEM, "text buffer allocation failed");
        HIPCHK(c, hipEventCreateWithFlags(&ev[i], hipEventDisableTiming));
    }
    for (size_t i = 0; i <= pieces.size(); i++) {
        if (i < pieces.size()) {  // format piece i while piece i - 1 is written
            const Piece& p = pieces[i];
            const int q = (int)(i % nbuf);
            const uint64_t len = off[p.b1] - off[p.b0];
            HIPCHK(c, launch_text(tv, cm, a, c->cfg.k, p.b0, p.b1 - p.b0, d_off, off[p.b0], d_txt[q], p.lds, c->stream));
            HIPCHK(c, hipMemcpyAsync(h_txt[q], d_txt[q], len, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipEventRecord(ev[q], c->stream));
        }
        if (i >= 1) {
            const Piece& p = pieces[i - 1];
            const int q = (int)((i - 1) % nbuf);
            const uint64_t len = off[p.b1] - off[p.b0];
            HIPCHK(c, hipEventSynchronize(ev[q]));
            if (std::fwrite(h_txt[q], 1, len, f) != len) return c->fail(KC_ERR_IO, "write failed");
        }
    }
    const int cl = std::fclose(file.release());
    if (cl != 0) return c->fail(KC_ERR_IO, "write failed");
    return KC_OK;
}

}  // extern "C"
