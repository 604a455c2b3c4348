// kc_api_path.cpp -- read paths through the compacted graph (include/kc_api.h kc_read_paths*): the
// checks, the scratch, the passes over the text and the host form.  The graph part is
// kc_unitig_graph*'s own host code (kc_api_unitig.cpp), which calls back here before its ranking
// (the scratch) and behind its last records launch (the text part).  Kernels: kc_path_impl.h (the
// place of every window) and kc_path.hip (run heads, ordered compaction, records, per-sequence
// sums); the cut into passes: kc_path_host.h.
#include "kc_ctx.h"
#include "kc_path_host.h"

#pragma GCC visibility push(hidden)

static_assert(sizeof(kc_path_run) == 32 && sizeof(kc_path_seq) == 32 && sizeof(kc_path_stats) == 64,
              "include/kc_api.h states these sizes");
static_assert(sizeof(kc_path_stats) == PATH_CTL_WORDS * sizeof(unsigned long long) &&
                  offsetof(kc_path_stats, runs) == PC_RUNS * 8 && offsetof(kc_path_stats, threaded) == PC_THREADED * 8,
              "kc_path_stats is the control words");
static_assert(sizeof(PathTile) == 32, "include/kc_api.h counts 32 bytes a tile");

struct PathText {
    const uint8_t* text;  // device
    uint64_t n;
    const uint64_t* offsets;  // host
    uint64_t n_seqs;
};

// kc_seq_stats_device's checks of the text
static int path_check_text(kc_ctx* c, const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t n_seqs) {
    if (n_seqs && !offsets) return c->fail(KC_ERR_ARG, "null offsets");
    for (uint64_t i = 0; i < n_seqs; i++)
        if (offsets[i] > offsets[i + 1]) return c->fail(KC_ERR_ARG, "sequence offsets decrease");
    if (n_seqs && offsets[n_seqs] > n) return c->fail(KC_ERR_ARG, "sequence offsets pass the end of the text");
    if (n_seqs && offsets[n_seqs] > offsets[0] && !text) return c->fail(KC_ERR_ARG, "null text");
    return KC_OK;
}

// the scratch of the text part; own_seq: the per-sequence records are the context's
static int path_reserve(kc_ctx* c, const PathText& t, const PathPlan& plan, bool own_seq) {
    const uint64_t n_off = t.n_seqs + 1, places = std::max<uint64_t>(1, plan.max_len), tiles = path_tiles(plan.max_len);
    const uint64_t n_seq = own_seq ? std::max<uint64_t>(1, t.n_seqs) : 0;
    if (c->d_path_place.capacity() < places || c->d_path_tiles.capacity() < tiles || c->d_seq_off.capacity() < n_off ||
        c->d_path_seq.capacity() < n_seq)
        make_room(c, places * 8 + tiles * sizeof(PathTile) + n_off * 8 + n_seq * sizeof(kc_path_seq));
    if (!c->d_path_place.reserve(places) || !c->d_path_tiles.reserve(tiles) || !c->d_path_ctl.reserve(PATH_CTL_WORDS) ||
        !c->h_seq_off.reserve(n_off) || !c->d_seq_off.reserve(n_off) || (n_seq && !c->d_path_seq.reserve(n_seq)))
        return c->fail(KC_ERR_NOMEM, "read paths: scratch allocation failed");
    return seq_stream_bufs(c, plan.max_len);
}

// The text part on s, behind the records launch that filled rec: every pass packs its text, finds
// the place of every window and compacts the runs behind the device's run cursor.  Outputs in
// device memory, each may be nullptr.  No host wait beyond an earlier call's offsets copy.
static int path_text_part(kc_ctx* c, const UnitigRanked& r, const uint32_t* rec, const PathText& t, const PathPlan& plan,
                          kc_path_run* runs, uint64_t cap_runs, kc_path_seq* seq, kc_path_stats* stats, hipStream_t s) {
    unsigned long long* ctl = c->d_path_ctl;
    HIPCHK(c, hipMemsetAsync(ctl, 0, PATH_CTL_WORDS * sizeof(unsigned long long), s));
    if (t.n_seqs) {
        kc_path_seq* sq = seq ? seq : c->d_path_seq.get();
        HIPCHK(c, hipMemsetAsync(sq, 0, t.n_seqs * sizeof(kc_path_seq), s));
        // the offsets go through pinned memory of the context, as kc_seq_stats_device's do
        const uint64_t n_off = t.n_seqs + 1;
        if (!c->seq_ev) HIPCHK(c, hipEventCreateWithFlags(&c->seq_ev, hipEventDisableTiming));
        HIPCHK(c, hipEventSynchronize(c->seq_ev));
        std::memcpy(c->h_seq_off, t.offsets, n_off * 8);
        HIPCHK(c, hipMemcpyAsync(c->d_seq_off, c->h_seq_off, n_off * 8, hipMemcpyHostToDevice, s));
        HIPCHK(c, hipEventRecord(c->seq_ev, s));
        const PackedView sv{c->d_seq_pk, c->d_seq_bk};
        const int k = c->cfg.k;
        for (const PathPassCut& p : plan.passes) {
            const uint64_t l0 = t.offsets[p.i0], len = t.offsets[p.i1] - l0;
            if (len >= (uint64_t)k) HIPCHK(c, launch_seq_pack(t.text + l0, len, sv, s));
            HIPCHK(c, launch_path_locate(table_view(c), sv, r.u, k, len, len, c->d_path_place, s));
            const PathPass pp{c->d_path_place, len, l0, c->d_seq_off, p.i0, p.i1, k};
            HIPCHK(c, launch_path_runs(pp, r.u, r.rounds, rec, c->d_path_tiles, runs, cap_runs, sq, ctl, s));
            HIPCHK(c, launch_path_finish(sq, p.i0, p.i1, ctl, s));
        }
    }
    if (stats) HIPCHK(c, hipMemcpyAsync(stats, ctl, sizeof(kc_path_stats), hipMemcpyDeviceToDevice, s));
    return KC_OK;
}

struct PathDevice final : UnitigAfter {
    PathText t;
    PathPlan plan;
    kc_path_run* runs;
    uint64_t cap_runs;
    kc_path_seq* seq;
    kc_path_stats* stats;
    int prepare(kc_ctx* c) override { return path_reserve(c, t, plan, !seq); }
    int run(kc_ctx* c, const UnitigRanked& r, const uint32_t* rec, hipStream_t s) override {
        return path_text_part(c, r, rec, t, plan, runs, cap_runs, seq, stats, s);
    }
};

// The host form's text part: the text to the device, the passes once without a run buffer for the
// number of runs, then with one of that size; waits.
struct PathHost final : UnitigAfter {
    const uint8_t* text;  // host
    uint64_t n;
    const uint64_t* offsets;
    uint64_t n_seqs;
    bool want_runs, want_seq;
    std::unique_ptr<kc_path_run, StdFree> out_runs;
    std::unique_ptr<kc_path_seq, StdFree> out_seq;
    kc_path_stats h{};
    int prepare(kc_ctx*) override { return KC_OK; }
    int run(kc_ctx* c, const UnitigRanked& r, const uint32_t* rec, hipStream_t s) override {
        const PathPlan plan = path_plan(offsets, n_seqs, c->batch_bytes);
        DevBuf<uint8_t> dt;
        DevBuf<kc_path_seq> ds;
        DevBuf<kc_path_run> dr;
        DrainOnError drain{s};
        const uint64_t used = n_seqs ? offsets[n_seqs] : 0;
        make_room(c, used + n_seqs * sizeof(kc_path_seq));
        if (!dt.reserve(std::max<uint64_t>(1, used)) || !ds.reserve(std::max<uint64_t>(1, n_seqs)))
            return c->fail(KC_ERR_NOMEM, "kc_read_paths: text and sequence buffer allocation failed");
        const PathText t{dt, used, offsets, n_seqs};
        int rc = path_reserve(c, t, plan, false);
        if (rc) return rc;
        if (used) HIPCHK(c, hipMemcpyAsync(dt, text, used, hipMemcpyHostToDevice, s));
        if ((rc = path_text_part(c, r, rec, t, plan, nullptr, 0, ds, nullptr, s))) return rc;
        HIPCHK(c, hipMemcpyAsync(&h, c->d_path_ctl, sizeof h, hipMemcpyDeviceToHost, s));
        HIPCHK(c, hipStreamSynchronize(s));
        if (want_runs && h.runs) {
            make_room(c, h.runs * sizeof(kc_path_run));
            if (!dr.reserve(h.runs)) return c->fail(KC_ERR_NOMEM, "kc_read_paths: run buffer allocation failed");
            if ((rc = path_text_part(c, r, rec, t, plan, dr, h.runs, ds, nullptr, s))) return rc;
        }
        if (want_runs) {
            out_runs.reset((kc_path_run*)std::malloc(std::max<size_t>(1, h.runs * sizeof(kc_path_run))));
            if (!out_runs) return c->fail(KC_ERR_NOMEM, "host allocation failed");
            if (h.runs) HIPCHK(c, hipMemcpyAsync(out_runs.get(), dr, h.runs * sizeof(kc_path_run), hipMemcpyDeviceToHost, s));
        }
        if (want_seq) {
            out_seq.reset((kc_path_seq*)std::malloc(std::max<size_t>(1, n_seqs * sizeof(kc_path_seq))));
            if (!out_seq) return c->fail(KC_ERR_NOMEM, "host allocation failed");
            if (n_seqs) HIPCHK(c, hipMemcpyAsync(out_seq.get(), ds, n_seqs * sizeof(kc_path_seq), hipMemcpyDeviceToHost, s));
        }
        HIPCHK(c, hipStreamSynchronize(s));
        drain.done();
        return KC_OK;
    }
};

#pragma GCC visibility pop

extern "C" {

int kc_read_paths_device(kc_ctx* c, uint32_t min_count, uint32_t max_count, kc_unitig* unitigs, uint64_t cap_unitigs,
                         uint8_t* bases, uint64_t cap_bases, kc_unitig_edge* edges, uint64_t cap_edges, kc_cdbg_stats* cdbg_stats,
                         const uint8_t* text, uint64_t n, const uint64_t* offsets, uint64_t n_seqs, kc_path_run* runs,
                         uint64_t cap_runs, kc_path_seq* seq, kc_path_stats* stats, void* sp) {
    if (!c) return KC_ERR_ARG;
    int rc = path_check_text(c, text, n, offsets, n_seqs);
    if (rc) return rc;
    if ((uintptr_t)runs & 15) return c->fail(KC_ERR_ARG, "kc_read_paths_device: dev_runs is not 16-byte aligned");
    if ((uintptr_t)seq & 7) return c->fail(KC_ERR_ARG, "kc_read_paths_device: dev_seq is not 8-byte aligned");
    PathDevice after;
    after.t = PathText{text, n, offsets, n_seqs};
    after.plan = path_plan(offsets, n_seqs, c->batch_bytes);
    after.runs = runs;
    after.cap_runs = cap_runs;
    after.seq = seq;
    after.stats = stats;
    return unitigs_device(c, true, min_count, max_count, unitigs, cap_unitigs, bases, cap_bases, edges, cap_edges, cdbg_stats,
                          (hipStream_t)sp, &after);
}

int kc_read_paths(kc_ctx* c, uint32_t min_count, uint32_t max_count, kc_unitig** unitigs, uint8_t** bases,
                  kc_unitig_edge** edges, kc_cdbg_stats* cdbg_stats, const uint8_t* text, uint64_t n, const uint64_t* offsets,
                  uint64_t n_seqs, kc_path_run** runs, kc_path_seq** seq, kc_path_stats* stats) {
    if (!c) return KC_ERR_ARG;
    if (runs) *runs = nullptr;
    if (seq) *seq = nullptr;
    if (unitigs) *unitigs = nullptr;
    if (bases) *bases = nullptr;
    if (edges) *edges = nullptr;
    int rc = path_check_text(c, text, n, offsets, n_seqs);
    if (rc) return rc;
    PathHost after;
    after.text = text;
    after.n = n;
    after.offsets = offsets;
    after.n_seqs = n_seqs;
    after.want_runs = runs != nullptr;
    after.want_seq = seq != nullptr;
    if ((rc = unitigs_host(c, true, min_count, max_count, unitigs, bases, edges, cdbg_stats, &after))) return rc;
    if (runs) *runs = after.out_runs.release();
    if (seq) *seq = after.out_seq.release();
    if (stats) *stats = after.h;
    return KC_OK;
}

}  // extern "C"
