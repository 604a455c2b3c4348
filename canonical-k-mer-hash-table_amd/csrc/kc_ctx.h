// kc_ctx.h -- private to the host side of the C ABI (kc_api*.cpp): the context, the owners of its
// device and pinned memory, the stream-and-profile scope of the device entry points, and the helpers
// the kc_api*.cpp files share.  Not part of the public boundary (that is include/kc_api.h).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/kc_api.h"
#include "kc_internal.h"
#include "kc_unitig_host.h"

// (nothing declared here is an export of libkc.so)
#pragma GCC visibility push(hidden)

using namespace kc;

// Owner of one allocation of T elements -- device memory (DevBuf) or pinned host memory (PinnedBuf:
// h_stage, h_desc, kc_write's text pieces) -- move-only, freed by its destructor.  It converts to
// the raw pointer, so launches, copies and the views the kernels receive (PartBufs, TableView,
// CompactView) read it like the T* it replaces.
struct DeviceMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static void free(void* p) { (void)hipFree(p); }
};
struct PinnedMem {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static void free(void* p) {
        if (p) (void)hipHostFree(p);
    }
};
template <class T, class Mem>
class OwnedBuf {
  public:
    OwnedBuf() = default;
    OwnedBuf(OwnedBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap_(std::exchange(o.cap_, 0)) {}
    OwnedBuf& operator=(OwnedBuf&& o) noexcept {  // (o's destructor frees what this one held)
        std::swap(p_, o.p_);
        std::swap(cap_, o.cap_);
        return *this;
    }
    ~OwnedBuf() { reset(); }

    // Grows only.  The old block is freed BEFORE the new one is allocated (next to a 100 GB table the
    // two do not fit side by side), so the contents are not kept.  false: the allocation failed and
    // the buffer is empty, capacity 0; the caller words its own KC_ERR_NOMEM.
    bool reserve(uint64_t n) {
        if (p_ && n <= cap_) return true;
        reset();
        if (Mem::alloc((void**)&p_, n * sizeof(T)) != hipSuccess) {
            p_ = nullptr;
            return false;
        }
        cap_ = n;
        return true;
    }
    void reset() {
        Mem::free(p_);
        p_ = nullptr;
        cap_ = 0;
    }
    T* get() const { return p_; }
    uint64_t capacity() const { return cap_; }  // elements
    operator T*() const { return p_; }
    T* operator->() const { return p_; }

  private:
    T* p_ = nullptr;
    uint64_t cap_ = 0;
};
template <class T>
using DevBuf = OwnedBuf<T, DeviceMem>;
template <class T>
using PinnedBuf = OwnedBuf<T, PinnedMem>;

// Buffers that grow together: all are freed before the first is allocated again
template <class... B>
void reset_all(B&... b) {
    (b.reset(), ...);
}
// (two of them: a failure leaves both empty, so that a's capacity() speaks for the pair)
template <class A, class B>
bool reserve_pair(A& a, uint64_t na, B& b, uint64_t nb) {
    if (a.get() && b.get() && na <= a.capacity() && nb <= b.capacity()) return true;
    reset_all(a, b);
    if (a.reserve(na) && b.reserve(nb)) return true;
    reset_all(a, b);
    return false;
}

// Declared after a call's temporaries, so that it runs before they are freed: a return that has
// not said done() -- an error return -- first waits for the async work that may still read them.
struct DrainOnError {
    hipStream_t s;
    bool armed = true;
    ~DrainOnError() {
        if (armed) (void)hipStreamSynchronize(s);
    }
    void done() { armed = false; }
};

// records on their way to the caller (who frees them with kc_free): an error return frees them
struct StdFree {
    void operator()(void* p) const { std::free(p); }
};
using HostRecords = std::unique_ptr<uint64_t, StdFree>;

// the histogram / offset arrays behind one PartBufs (the view the kernels receive holds their
// pointers; capacities in entries: off1 hist1 + 1, off2 hist2 + 1)
struct PartHist {
    DevBuf<uint32_t> hist1, hist2;
    DevBuf<uint64_t> off1, off2, bsum;
};

#pragma GCC visibility pop

// (default visibility, as it always had: its inline members are weak exports of libkc.so)
struct kc_ctx {
    kc_config cfg{};
    int W = 1, S = 8;
    hipStream_t stream = nullptr;
    std::string err;

    // staging
    uint64_t batch_bytes = 0;
    uint64_t max_chunks = 0;
    PinnedBuf<uint8_t> h_stage[2];
    PinnedBuf<ChunkDesc> h_desc[2];
    hipEvent_t h_free[2] = {nullptr, nullptr};  // recorded after the H2D reading buffer i
    hipEvent_t xev = nullptr;                   // orders the context stream with a caller stream
    hipStream_t aux = nullptr;                  // the kept Bloom batch's checksum, beside its levels
    hipEvent_t aev[2] = {nullptr, nullptr};     // caller stream -> aux -> caller stream
    int cur = 0;
    uint64_t cur_used = 0;                      // stage bytes used in h_stage[cur]
    uint64_t cur_n = 0;                         // chunks in h_stage[cur]
    int cur_fmt = -1;
    int cur_pass = -1;                          // 0 count, 1 bloom

    DevBuf<uint8_t> d_stage;
    DevBuf<uint64_t> d_pk;  // packed symbol stream
    DevBuf<uint32_t> d_bk;  // break bitmap
    DevBuf<TileInfo> d_tiles;
    DevBuf<TileOut> d_touts;
    DevBuf<TileOut> d_tblk;  // per-1024-tile block prefixes
    DevBuf<ChunkDesc> d_chunks;
    DevBuf<DevCounters> d_ctr;

    // table
    DevBuf<uint64_t> d_table;  // (its capacity: a Bloom job re-sizes the table per pass)
    uint64_t nbuckets = 0;
    uint64_t R = 0;
    uint32_t F1 = 1, F2 = 1;
    int f2bits = 0;
    bool seg_ok = true;  // the table's geometry fits the segmented single-pass levels (else exact layout)

    // partitioned insert buffers (pb: the table's levels; pbf: the Bloom pass's, same key
    // buffers, own histograms)
    PartBufs pb{}, pbf{};
    PartHist pb_own, pbf_own;
    DevBuf<uint64_t> d_keys1, d_keys2;  // the level-1 / level-2 key buffers (u64 words)
    DevBuf<uint64_t> d_spill;           // skew list of a segmented batch (ensure_part_geo)
    bool table_fresh = false;  // the table is all zero (allocated / reset, nothing inserted since)
    uint64_t min_slots = 0;        // the job's -s (or 2 * new_in_second): the reference's table size
    bool strict_capacity = false;  // KC_STRICT_CAPACITY=1: fail past the reference's capacity
    // kc_reset defers the table memset: a fresh level-3 pass writes every region anyway;
    // any other use of the table zeroes it first (materialize_zero)
    bool table_zero_pending = false;
    // kc_route_table_device: per-(owner, block) record counts, their scan, scan scratch
    DevBuf<uint32_t> d_rhist;
    DevBuf<uint64_t> d_roff;
    DevBuf<uint64_t> d_rbsum;
    // kc_route_hint: the level-3 passes keep d_rhist for own_parts owners (PartBufs.own_hist);
    // own_valid = it holds the table's current per-block record counts
    uint32_t own_parts = 0;
    bool own_valid = false;
    uint64_t route_counts_kept = 0;  // kc_route_table_device calls that skipped the count pass
    // kc_insert_counts_runs_device: group offsets, region run starts / lengths
    DevBuf<uint64_t> d_gstart;
    DevBuf<uint64_t> d_mstart;
    DevBuf<uint32_t> d_mlen;

    // bloom
    DevBuf<uint32_t> d_bloom;
    uint64_t bf_bits = 0;
    int nh = 0, nh_gate = 0;
    int bloom_blocked = 1;  // KC_BLOOM_LAYOUT=reference: the reference's independent positions
    bool bloom_final = false;
    bool bloom_fresh = false;  // the filter is all zero (allocated / reset, nothing inserted since)
    TableView bgeo{};          // blocked layout: the filter's region geometry (k_b3 regions)

    // Level-1 reuse (device path): a Bloom job whose Bloom pass is ONE batch over a device
    // image keeps that pass's level-1 output (whole table keys in the filter's coarse bins,
    // launch_bloom_partitioned keep); the table is then sized with the same coarse bins, and
    // a counting pass over the same image and chunks (checked: pointer, chunk list, format
    // and a checksum of the bytes) starts at level 2 instead of tokenizing and extracting
    // every window again (launch_count_reuse).  KC_REUSE=0 disables it.
    int bloom_batches = 0;            // Bloom-pass batches since the job started
    bool reuse_kept = false;          // the (only) Bloom batch kept its level-1 output
    bool reuse_ok = false;            // kc_bloom_finalize: kept, no skew entries, geometry fits
    const uint8_t* reuse_img = nullptr;  // borrowed: the caller's image, compared, never read through
    std::vector<ChunkDesc> reuse_chunks;
    int reuse_fmt = -1;
    uint64_t reuse_used = 0;          // stage bytes of the batch
    unsigned long long reuse_sum = 0; // checksum of the Bloom pass's chunk bytes
    uint64_t reuse_windows = 0;       // windows of that batch
    DevBuf<unsigned long long> d_sum;  // CHECKSUM_SLOTS partial sums (+ CHECKSUM_SLOTS for kc_bloom_estimate)
    // the counting pass's checksum of its bytes, copied back on the aux stream: context memory, so
    // a call that returns before waiting for that copy leaves it no dangling destination
    unsigned long long h_part[CHECKSUM_SLOTS] = {};
    DevBuf<uint32_t> d_hll;            // HLL_M registers of kc_estimate_distinct_device
    // compact representation (kc_compact): slot words, chain-start keys, counters
    DevBuf<uint64_t> d_cwords;
    uint64_t cslots = 0;
    DevBuf<uint64_t> d_csecond;
    uint64_t cstarts = 0, ckmers = 0;
    DevBuf<unsigned long long> d_cstat;  // [0] chain starts / record cursor, [1] hops, [2] max hops, [3] bad walks
    DevBuf<uint32_t> d_keep_fill;      // the kept partitions' segment fills: level 1 [F1][nblk1]
    DevBuf<uint32_t> d_keep_fill2;     // and level 2 [R_fine][B2]
    TableView fgeo{};                     // the kept partitions' fine geometry (powers of two)
    uint64_t fgeo_max_R = 0;              // the create-time fine regions (the most the LDS fits)
    uint64_t fgeo_next_R = 0;             // fine regions learned from the last finalize (0 = keep)
    int reuse_level = 0;                  // kc_bloom_finalize: 2 = from level 2, 1 = from level 1
    uint64_t reuse_hits = 0;          // counting passes that reused (kc_stats.reused_passes)
    int reuse_last_level = 0;         // the level the last reused pass started from (kc_stats.reuse_level)

    // sequence queries (kc_api_seq.cpp): one pass's packed stream and per-position counts, the
    // sequences' offsets followed by the ids of the long ones (device copy and the pinned block it is
    // copied from; seq_ev: that copy has read the pinned block)
    DevBuf<uint64_t> d_seq_pk;
    DevBuf<uint32_t> d_seq_bk;
    DevBuf<uint32_t> d_seq_cnt;
    DevBuf<uint64_t> d_seq_off;
    PinnedBuf<uint64_t> h_seq_off;
    hipEvent_t seq_ev = nullptr;
    // read correction (kc_api_correct.cpp): a verdict byte per position of a pass, beside the
    // sequence queries' stream, counts and offsets
    DevBuf<uint8_t> d_cor_vd;
    // the de Bruijn graph (kc_api_graph.cpp): an edge byte per table slot, and the statistics words
    // followed by the record cursor (GRAPH_STAT_WORDS)
    DevBuf<uint8_t> d_graph_edges;
    DevBuf<unsigned long long> d_graph_stat;
    // the unitigs (kc_api_unitig.cpp): a node id per table slot, the per-node arrays of UnitigBufs in
    // one block (unitig_layout), the control words; they grow only.  d_unitig_rec: the record index
    // per node id, allocated by kc_unitig_graph* alone
    DevBuf<uint32_t> d_unitig_ids;
    DevBuf<uint64_t> d_unitig_node;
    DevBuf<unsigned long long> d_unitig_ctl;
    DevBuf<uint32_t> d_unitig_rec;
    // read paths (kc_api_path.cpp): a place per position of a pass, the tiles' run heads, the control
    // words (kc_path_stats), and the per-sequence records of a call without dev_seq; beside the
    // sequence queries' stream and offsets
    DevBuf<uint2> d_path_place;
    DevBuf<PathTile> d_path_tiles;
    DevBuf<unsigned long long> d_path_ctl;
    DevBuf<kc_path_seq> d_path_seq;

    uint64_t n_chunks = 0, n_bytes = 0;

    // Deferred level 3 (device_pass / run_deferred): a counting pass over an image of several
    // batches keeps the level-2 segments of up to defer_g batches in keys2 and inserts them with one
    // level-3 pass -- one sweep of the table per group instead of per batch
    bool defer_on = false;     // the current device_pass defers (set per pass)
    bool defer_last = false;   // the batch being launched is the pass's last
    uint32_t defer_g = 0;      // batches per group
    uint32_t defer_n = 0;      // batches of the current group whose segments wait
    uint64_t skew_prev = 0;    // the group's skew list after its last batch (entries, of them records of
    uint64_t heavy_prev = 0;   // repeated windows): what a batch that overflows leaves to insert
    uint64_t defer_syms = 0;   // the group's segment geometry is sized for batches of this bound
    uint64_t defer_groups = 0; // level-3 passes the deferral ran (kc_stats)
    // super-k-mer routing (kc_route_superkmers_device): the pass-4 batches' parameters and the
    // device cursors [0, 64) words per owner, [64, 128) windows per owner, [128] overflow flag
    DevBuf<unsigned long long> d_skm;
    DevBuf<unsigned long long> d_pwin;  // a packed pass's counted windows per batch (k_packed_windows)
    uint32_t skm_shards = 0;
    int skm_m = 0;
    uint64_t* skm_pk = nullptr;  // borrowed: the caller's output streams, for the length of
    uint32_t* skm_bk = nullptr;  // the call
    uint64_t skm_cap = 0;
    // kc_estimate_distinct_device keeps its tokenized batches for the next counting pass over the
    // same image, chunks and format (kept_*): keep_pk / keep_bk hold batch i's stream at word kept[i].first
    // (both of keep_pk's capacity in words)
    DevBuf<uint64_t> keep_pk;
    DevBuf<uint32_t> keep_bk;
    uint64_t keep_woff = 0;                // words used
    bool keep_target = false;              // the estimate pass writes its streams there
    bool kept_valid = false;
    const uint8_t* kept_img = nullptr;  // borrowed: the caller's image, compared, never read through
    int kept_fmt = -1;
    std::vector<kc_chunk> kept_chunks;
    std::vector<std::pair<uint64_t, uint64_t>> kept;  // per batch: first word, symbol bound
    DevBuf<uint64_t> d_kept_len;                       // per batch: the stream length the tokenizer left
    DevBuf<uint64_t> d_kept_win;                       // per batch: the estimate pass's windows so far
    double kept_density = 1.0;                         // the kept batches' largest windows per symbol
    // windows per symbol of the batches being planned (1: tokenized input, where every symbol can
    // end a window; a received super-k-mer stream carries k symbols of context per run)
    double win_density = 1.0;
    // a counting pass failed after some of its batches were counted (a deferred group whose level 3
    // never ran, a failed launch): the table no longer matches the windows counted, so every call
    // that counts or reads the table fails until kc_reset
    std::string broken;

    // profiling: event quadruples {start, after gather, after tokenize, after count}
    bool profiling = false;
    std::vector<hipEvent_t> ev_pool;
    std::vector<std::array<hipEvent_t, 4>> ev_pending;
    kc_timing timing{};

    hipEvent_t get_event() {
        if (!ev_pool.empty()) {
            hipEvent_t e = ev_pool.back();
            ev_pool.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }

    int fail(int code, const std::string& m) {
        err = m;
        return code;
    }
    int hipfail(hipError_t e, const char* what) {
        err = std::string(what) + ": " + hipGetErrorString(e);
        return KC_ERR_HIP;
    }
};

#pragma GCC visibility push(hidden)

#define HIPCHK(ctx, expr)                                  \
    do {                                                   \
        hipError_t _e = (expr);                            \
        if (_e != hipSuccess) return (ctx)->hipfail(_e, #expr); \
    } while (0)

// the calls that count into or read the table refuse a job a failed pass left incomplete
#define JOB_OK(ctx)                                                                            \
    do {                                                                                       \
        if (!(ctx)->broken.empty()) return (ctx)->fail(KC_ERR_STATE, (ctx)->broken + " (kc_reset first)"); \
    } while (0)

// A profiling quadruple while it is being recorded.  commit() hands it to ev_pending
// (kc_get_timing reads it and returns its events to the pool); one that is dropped first, on an
// error or a path that times nothing, returns its events to ev_pool itself.
struct ProfEvents {
    kc_ctx* c;
    std::array<hipEvent_t, 4> ev{};
    explicit ProfEvents(kc_ctx* c) : c(c) {}
    ProfEvents(const ProfEvents&) = delete;
    ProfEvents& operator=(const ProfEvents&) = delete;
    ~ProfEvents() {
        for (auto e : ev)
            if (e) c->ev_pool.push_back(e);
    }
    void take(int i) { ev[i] = c->get_event(); }
    void commit() {
        c->ev_pending.push_back(ev);
        ev.fill(nullptr);
    }
};

// The device entry points run on the caller's stream s, ordered after the work already enqueued
// there (NULL = the HIP null stream, PyTorch's default current stream), and hand over to/from the
// context's own stream with events.  One scope per call, built after flush_host:
//   join()     s waits for the context's stream (nothing when they are the same stream)
//   profile()  opens the {ev[2], ev[3]} bracket of a call that is not a full batch (profiling only)
//   finish()   the success path: ev[3] is recorded, the bracket joins ev_pending, then the context's
//              stream waits for s
// A scope left any other way -- an error return -- still hands the context's stream back and returns
// its events to the pool; what HIP says then does not replace the error being returned.
struct StreamScope {
    kc_ctx* c;
    hipStream_t s;
    bool joined = false;
    ProfEvents prof;
    StreamScope(kc_ctx* c, hipStream_t s) : c(c), s(s), prof(c) {}
    StreamScope(const StreamScope&) = delete;
    StreamScope& operator=(const StreamScope&) = delete;
    ~StreamScope() {
        if (!joined) return;
        std::string err = std::move(c->err);
        (void)hand_back();
        c->err = std::move(err);
    }
    int join() {
        if (s == c->stream || joined) return KC_OK;
        joined = true;
        HIPCHK(c, hipEventRecord(c->xev, c->stream));
        HIPCHK(c, hipStreamWaitEvent(s, c->xev, 0));
        return KC_OK;
    }
    int profile() {
        if (!c->profiling) return KC_OK;
        auto& ev = prof.ev;
        prof.take(2);
        prof.take(3);
        HIPCHK(c, hipEventRecord(ev[2], s));
        return KC_OK;
    }
    int end_profile() {
        auto& ev = prof.ev;
        if (!ev[3]) return KC_OK;
        HIPCHK(c, hipEventRecord(ev[3], s));
        prof.commit();
        return KC_OK;
    }
    int hand_back() {
        if (!joined) return KC_OK;
        joined = false;
        HIPCHK(c, hipEventRecord(c->xev, s));
        HIPCHK(c, hipStreamWaitEvent(c->stream, c->xev, 0));
        return KC_OK;
    }
    int finish() {
        const int rc = end_profile();
        return rc ? rc : hand_back();
    }
    // A success path that never handed back: the call has waited for s itself, or it counted
    // nothing and the ordinary pass that follows joins again.
    void no_hand_back() { joined = false; }
};

// ---- helpers shared by the kc_api*.cpp files (defined in the file named) -------------------------
inline uint64_t round_up(uint64_t v, uint64_t a) { return (v + a - 1) / a * a; }

// (PartGeo, PartPlan: kc_plan_host.h)
inline PartGeo table_geo(const kc_ctx* c) { return PartGeo{c->F1, c->F2, c->R, c->W}; }

// kc_api.cpp
uint64_t bloom_blocks(uint64_t bits);
uint64_t bloom_words(const kc_ctx* c);
int route_bufs(kc_ctx* c, uint64_t n);
int own_prep(kc_ctx* c);
void own_after_write(kc_ctx* c, bool level3, bool fresh);
int alloc_table(kc_ctx* c, uint64_t min_slots, uint32_t pow2_f1 = 0, uint64_t phys_slots = 0);
TableView table_view(const kc_ctx* c);
int materialize_zero(kc_ctx* c, hipStream_t s);
PartPlan part_plan(const kc_ctx* c, uint64_t syms, bool seg, const PartGeo& g, uint32_t bins1, uint32_t slots,
                   uint64_t rec2 = 0, bool tight = false);
int ensure_part_geo(kc_ctx* c, uint64_t syms, bool seg, const PartGeo& g, PartBufs& pb, PartHist& own,
                    uint32_t bins1 = 0, uint32_t slots = 1, uint64_t rec2 = 0);
int ensure_part(kc_ctx* c, uint64_t syms, bool seg, uint32_t bins1 = 0, uint32_t slots = 1);
enum class PathKnob { Auto, Direct, Partitioned, Exact };
PathKnob insert_path_knob();
bool debug_on();
bool use_partitioned(const kc_ctx* c, uint64_t syms);
bool use_partitioned_bloom(const kc_ctx* c, uint64_t syms);
int sync_for_read(kc_ctx* c);
void make_room(kc_ctx* c, uint64_t bytes);
void drop_compact(kc_ctx* c);
// kc_api_unitig.cpp (shared with kc_api_filter.cpp: the checks, the ids' bound of a host form, the
// ranking).  A ranking leaves the views of the context's scratch, the jump rounds the later launches
// repeat, and the anchors behind the verdict bytes (nullptr unless wanted)
struct UnitigRanked {
    UnitigBufs u;
    int rounds;
    uint32_t* anchors;
};
int unitig_check(kc_ctx* c, uint32_t min_count, uint32_t max_count);
int unitig_bound(kc_ctx* c, uint32_t min_count, unsigned long long* bound);
int unitig_rank(kc_ctx* c, uint32_t min_count, uint32_t max_count, uint64_t bound, UnitigWants w, hipStream_t s,
                UnitigRanked* r);
// What kc_read_paths* (kc_api_path.cpp) adds to the compacted graph's call: prepare reserves its
// scratch before the ranking's first kernel (the device form), run enqueues its work behind the
// call's last records launch, whose numbering rec holds.
struct UnitigAfter {
    virtual int prepare(kc_ctx* c) = 0;
    virtual int run(kc_ctx* c, const UnitigRanked& r, const uint32_t* rec, hipStream_t s) = 0;

  protected:
    ~UnitigAfter() = default;
};
int unitigs_device(kc_ctx* c, bool with_edges, uint32_t min_count, uint32_t max_count, kc_unitig* unitigs,
                   uint64_t cap_unitigs, uint8_t* bases, uint64_t cap_bases, kc_unitig_edge* edges, uint64_t cap_edges,
                   void* stats, hipStream_t s, UnitigAfter* after);
int unitigs_host(kc_ctx* c, bool with_edges, uint32_t min_count, uint32_t max_count, kc_unitig** unitigs, uint8_t** bases,
                 kc_unitig_edge** edges, void* stats, UnitigAfter* after);
// kc_api_seq.cpp: the packed stream of a pass of up to n bytes
int seq_stream_bufs(kc_ctx* c, uint64_t n);
// kc_api_pass.cpp
int flush_host(kc_ctx* c);
int device_pass(kc_ctx* c, const uint8_t* img, const kc_chunk* chunks, size_t n, int fmt, int pass, hipStream_t s);

// What the record / key inserts (kc_api_shard.cpp) and the table algebra (kc_api_join.cpp) share, on
// the caller's stream (joined here unless the caller has): `size` prepares the partition buffers (or
// the table), before the profiling bracket opens or (prof_first) after it; `work` is the launch the
// bracket times; then the table's -- or (bloom) the filter's -- freshness flags.
template <class Size, class Work>
int insert_on(kc_ctx* c, StreamScope& on, bool bloom, bool prof_first, Size size, Work work) {
    int rc = on.join();
    if (rc) return rc;
    if (prof_first && (rc = on.profile())) return rc;
    if ((rc = size())) return rc;
    if (!prof_first && (rc = on.profile())) return rc;
    if ((rc = work())) return rc;
    if (bloom) {
        c->bloom_fresh = false;
    } else {
        own_after_write(c, false, false);
        c->table_fresh = c->table_zero_pending = false;
    }
    return on.finish();
}

// ---- what every call on two or three contexts shares (kc_api_join.cpp, kc_api_filter.cpp) ----------
// The error of a step on `from` is reported on the context the caller reads: dst, else the first operand.
inline int route_rc(kc_ctx* err, kc_ctx* from, int rc) {
    if (rc && from != err) err->err = from->err;
    return rc;
}

// The write into dst on s: dst's host-side state as after kc_insert_counts_device's direct insert
// (the compact representation is a snapshot of the table before this call, so it goes), dst zeroed
// if that is pending, then `work`, the launches that insert.  Without a dst, `work` alone.
template <class Work>
int write_dst(kc_ctx* dst, hipStream_t s, Work work) {
    if (!dst) return work();
    if (dst->d_cwords) drop_compact(dst);
    StreamScope on_d(dst, s);
    return insert_on(dst, on_d, false, true, [&] { return materialize_zero(dst, s); }, work);
}

// The host form of a call whose only output is a statistics struct: body(device struct or nullptr,
// stream) is the device form, on the stream of the context that reports the error; then the copy
// back and the wait -- also after an error, since the kernels may still write the struct.
template <class Stats, class Body>
int stats_host_form(kc_ctx* err, const char* name, Stats* stats, Body body) {
    DevBuf<Stats> d;
    if (stats && !d.reserve(1)) return err->fail(KC_ERR_NOMEM, std::string(name) + ": statistics allocation failed");
    hipStream_t s = err->stream;
    int rc = body(d.get(), s);
    hipError_t e = hipSuccess;
    if (rc == KC_OK && stats) e = hipMemcpyAsync(stats, d, sizeof(Stats), hipMemcpyDeviceToHost, s);
    const hipError_t e2 = hipStreamSynchronize(s);
    if (rc == KC_OK && (e != hipSuccess || e2 != hipSuccess))
        rc = err->hipfail(e != hipSuccess ? e : e2, (std::string(name) + ": statistics copy").c_str());
    return rc;
}

#pragma GCC visibility pop
