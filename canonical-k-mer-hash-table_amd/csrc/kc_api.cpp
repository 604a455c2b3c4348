// kc_api.cpp -- host side of the C ABI (include/kc_api.h): the context's life (create, destroy,
// reset, finish, sync, stats, timing) and the table / Bloom / partition-buffer sizing every pass
// shares.  The passes are in kc_api_pass.cpp, the sharded entry points in kc_api_shard.cpp, the
// readers in kc_api_read.cpp, the chunk planner in kc_api_plan.cpp; kc_ctx.h holds what they share.
// All compiled by hipcc into libkc.so together with the kernels.
//
// Data flow per batch (the reference's io_worker -> in_queue -> string_worker,
// parallel_parser.hpp:1230-1519, re-shaped for one device):
//   host chunk -> pinned stage image (chunk at a 4 KiB-aligned offset)
//   -> one async H2D per batch -> tokenize (3 kernels) -> count/bloom kernel.
// Two pinned stage buffers alternate so the host fills one while the device
// consumes the other.
#include "kc_ctx.h"

namespace {

thread_local std::string g_create_error;

constexpr uint64_t kDefaultBatch = 256ull << 20;

}  // namespace

// ------------------------------------------------------------------------------
// sizing helpers
// ------------------------------------------------------------------------------
static void bloom_sizes(uint64_t U, double fpr, uint64_t* bits, int* nh, int* nh_gate) {
    // main.cpp:402-418: bits = next pow2 >= -U ln f / ln^2 2 (compared as uint64),
    // hf = bits_min / U * ln 2; pass 1 uses ceil(hf) (main.cpp:417), the pass-2 gate
    // receives hf through a uint64_t parameter, i.e. trunc(hf) (parallel_parser.hpp:2397).
    double bits_min = (-double(U) * std::log(fpr)) / std::pow(std::log(2), 2);
    double hf = (bits_min / double(U)) * std::log(2);
    uint64_t b = 2;
    while (b < uint64_t(bits_min)) b *= 2;
    *bits = b;
    *nh = int(std::ceil(hf));
    *nh_gate = int(uint64_t(hf));
}

// blocked layout: 512-bit blocks holding 256 positions of both filters
uint64_t bloom_blocks(uint64_t bits) { return std::max<uint64_t>(1, bits / 256); }

uint64_t bloom_words(const kc_ctx* c) {
    const uint64_t w = std::max<uint64_t>(1, (2 * c->bf_bits + 31) / 32);
    return c->bloom_blocked ? std::max<uint64_t>(w, 16 * bloom_blocks(c->bf_bits)) : w;
}

static int alloc_regions(kc_ctx* c);

// kc_route_table_device's buffers for n = parts x blocks entries (d_rhist moves: the level-3
// passes' pointer follows it and the kept counts are gone)
int route_bufs(kc_ctx* c, uint64_t n) {
    if (n <= c->d_rhist.capacity()) return KC_OK;
    reset_all(c->d_rhist, c->d_roff, c->d_rbsum);
    c->own_valid = false;
    c->pb.own_hist = c->pbf.own_hist = nullptr;
    c->pb.own_parts = c->pbf.own_parts = 0;
    if (!c->d_rhist.reserve(n) || !c->d_roff.reserve(n + 1) || !c->d_rbsum.reserve((n + 4095) / 4096 + 2)) {
        reset_all(c->d_rhist, c->d_roff, c->d_rbsum);
        return c->fail(KC_ERR_NOMEM, "route buffers allocation failed");
    }
    return KC_OK;
}

// Point the level-3 passes at d_rhist for the table's current geometry (kc_route_hint); the
// counts are valid again after a fresh level-3 pass (which writes every region)
int own_prep(kc_ctx* c) {
    c->own_valid = false;
    c->pb.own_hist = c->pbf.own_hist = nullptr;
    c->pb.own_parts = c->pbf.own_parts = 0;
    if (!c->own_parts || !c->nbuckets) return KC_OK;
    const uint64_t nblk = (c->nbuckets + 255) / 256;  // = 2 R (BPR = 512)
    const int rc = route_bufs(c, c->own_parts * nblk);
    if (rc) return rc;
    c->pb.own_hist = c->pbf.own_hist = c->d_rhist;
    c->pb.own_parts = c->pbf.own_parts = c->own_parts;
    c->pb.own_nblk = c->pbf.own_nblk = nblk;
    return KC_OK;
}

// After a write into the table: the kept per-block counts stay valid through level-3 passes
// (k_p3 rewrites the counts of every region it writes; a fresh pass writes every region) and
// are lost by any other writer (direct atomics, the merge inserts)
void own_after_write(kc_ctx* c, bool level3, bool fresh) {
    if (!level3) c->own_valid = false;
    else if (fresh) c->own_valid = c->pb.own_parts != 0;
}

// pow2_f1 != 0: R = F1 x F2 with F1 = pow2_f1 (the Bloom filter's coarse bins) and F2 a power
// of two, so the table's coarse bins are the filter's hash-prefix bins (level-1 reuse)
// phys_slots != 0: size the device table for that many k-mers instead of min_slots (the
// reference's capacity stays min_slots: kc_stats, KC_STRICT_CAPACITY)
int alloc_table(kc_ctx* c, uint64_t min_slots, uint32_t pow2_f1, uint64_t phys_slots) {
    c->min_slots = min_slots;
    // Kaarme's table holds exactly next_prime3mod4(min_slots) slots and dies when
    // full; open addressing on the GPU keeps 25 % headroom over that.  The table is
    // R = F1 * F2 regions of BPR 128-byte buckets (a region = one LDS-resident table).
    uint64_t want = std::max<uint64_t>(phys_slots ? phys_slots : min_slots, 64);
    want = want + want / 4;
    const uint64_t buckets = (want + c->S - 1) / c->S;
    const uint64_t regions = std::max<uint64_t>(1, (buckets + BPR - 1) / BPR);
    // R = F1 * F2 regions: F2 = 2^f2bits regions per level-1 bin, F1 ~ sqrt(R) <= 1024 bins
    // (multiply-shift region index, so R is not rounded up to a power of two)
    int rbits = 0;
    while ((1ULL << rbits) < regions) rbits++;
    if (pow2_f1) {
        int f1 = 0;
        while ((1u << f1) < pow2_f1) f1++;
        c->f2bits = std::max(0, rbits - f1);
        c->F2 = 1u << c->f2bits;
        c->F1 = pow2_f1;
        c->seg_ok = true;
    } else {
        // level 1 keeps F1 bins' arrays beside its tile in LDS (p1_lds_bytes), level 2 F2 bins'
        // (p2f_lds_bytes): big tables (C4, C5 shares) take more regions per coarse bin until
        // level 2 fits; for wide keys, if level 1 then does not fit, fewer, with level 2 at half
        // its workgroup (launch_p2f)
        auto f1_of = [&](int f2b) { return (uint32_t)((regions + (1ULL << f2b) - 1) >> f2b); };
        auto l2_fits = [&](int f2b, int nt) {
            const uint64_t b2 = std::max<uint64_t>(1, std::min<uint64_t>(64, 2048 / std::max<uint32_t>(1, f1_of(f2b))));
            return p2f_lds_bytes(c->W, 1u << f2b, (uint32_t)((2048 + b2 - 1) / b2), nt) <= LDS_BYTES;
        };
        auto l1_fits = [&](int f2b) { return p1_lds_bytes(c->W, f1_of(f2b)) <= LDS_BYTES; };
        int f1bits = std::min(10, (rbits + 1) / 2);
        while (f1bits < rbits && !l2_fits(rbits - f1bits, 0)) f1bits++;
        // level-1 runs of fewer than 8 keys per tile cost level 1 its second workgroup per CU
        // (launch_part_w): fewer, wider coarse bins while level 2 still fits (C4 share: 542 x 512
        // -> 271 x 1024 bins, k_p1 14.9 -> 9.9 ms, k_p2f 11.0 -> 12.3 ms, r03_ab_c4s_coarse_bins.txt)
        while (f1bits > 1 && (uint64_t)p1_tile(c->W) < 8ULL * f1_of(rbits - f1bits) &&
               l2_fits(rbits - f1bits + 1, 0))
            f1bits--;
        c->seg_ok = true;
        if (!l1_fits(rbits - f1bits)) {
            const int half = p2f_threads_w(c->W) / 2;
            f1bits = std::min(10, (rbits + 1) / 2);
            while (f1bits > 0 && !l1_fits(rbits - f1bits)) f1bits--;
            if (c->W <= 2 || !l1_fits(rbits - f1bits) || !l2_fits(rbits - f1bits, half)) {
                // beyond the segmented levels (wide keys in a multi-G-slot table, e.g. C5 on one
                // GPU): the exact layout, whose 256-thread levels hold smaller tiles
                const size_t tile = (size_t)COUNT_THREADS * run_width(c->W) * 8 * c->W + 16;
                auto fits_x = [&](uint64_t bins) { return bins * 32 + tile <= LDS_BYTES; };
                f1bits = 0;
                while (f1bits <= rbits && !(fits_x(f1_of(rbits - f1bits)) && fits_x(1ULL << (rbits - f1bits)))) f1bits++;
                if (f1bits > rbits) return c->fail(KC_ERR_ARG, "table too large for the partition levels");
                c->seg_ok = false;
            }
        }
        c->f2bits = rbits - f1bits;
        c->F2 = 1u << c->f2bits;
        c->F1 = f1_of(c->f2bits);
        // one-word keys: the level-2 records are 6 instead of 8 bytes once R >= 2^16
        // (kc_count_impl.h StoreRec6), so a table of 3/4 x 2^16 regions or more takes 2^16
        // (C2's -s 2e8: 61 184 -> 65 536 regions, 7 % more slots for 25 % fewer level-2 bytes)
        const uint64_t r0 = (uint64_t)c->F1 * c->F2;
        if (c->W == 1 && c->seg_ok && r0 >= 49152 && r0 < 65536 && l1_fits(c->f2bits)) {
            const uint32_t f1 = (uint32_t)((65536 + c->F2 - 1) / c->F2);
            if (p1_lds_bytes(1, f1) <= LDS_BYTES) c->F1 = f1;
        }
    }
    c->R = (uint64_t)c->F1 * c->F2;
    return alloc_regions(c);
}

// the table's memory for c->R regions (the geometry set by the caller)
static int alloc_regions(kc_ctx* c) {
    if (c->R >= (1ULL << 32)) return c->fail(KC_ERR_ARG, "table too large");  // 32-bit region index (kc_common.h)
    c->nbuckets = c->R * BPR;
    const size_t bytes = c->nbuckets * BUCKET_WORDS * sizeof(uint64_t);
    if (!c->d_table.reserve(bytes / sizeof(uint64_t)))  // (a previous allocation that is large enough stays)
        return c->fail(KC_ERR_NOMEM, "table allocation failed (" + std::to_string(bytes) + " bytes)");
    // zeroed lazily: a fresh partitioned pass writes every region from zero-filled LDS (C3's
    // counting pass: 0.66 ms of its 31 ms step was this memset), anything else that reads the
    // table first runs materialize_zero
    c->table_zero_pending = true;
    c->table_fresh = true;
    return own_prep(c);
}

TableView table_view(const kc_ctx* c) {
    TableView tv;
    tv.buckets = c->d_table;
    tv.nbuckets = c->nbuckets;
    tv.R = c->R;
    tv.F1 = c->F1;
    tv.F2 = c->F2;
    tv.f2bits = c->f2bits;
    tv.W = c->W;
    tv.S = c->S;
    return tv;
}

// Perform a deferred table reset before the table is read or updated by anything but a
// fresh level-3 pass.
int materialize_zero(kc_ctx* c, hipStream_t s) {
    if (!c->table_zero_pending || !c->d_table) return KC_OK;
    HIPCHK(c, hipMemsetAsync(c->d_table, 0, c->nbuckets * BUCKET_WORDS * sizeof(uint64_t), s));
    c->table_zero_pending = false;
    return KC_OK;
}

// Partition buffers for a batch of up to `syms` symbols (lazily grown).  seg: use the
// segmented single-pass layout (fixed-capacity segments, kc_count.hip OutSeg); its
// capacities are the expected fill of a segment (keys are hash-uniform over bins) plus
// 8 standard deviations plus 32, from the batch's symbol bound (>= its windows).  A
// batch whose keys still overflow a segment (e.g. one k-mer repeated millions of times
// inside one workgroup's range) is redone on the exact layout by the device itself.
// The arithmetic is plan_partition (kc_plan_host.h); the tests' knobs are read here.
PartPlan part_plan(const kc_ctx* c, uint64_t syms, bool seg, const PartGeo& g, uint32_t bins1, uint32_t slots,
                   uint64_t rec2, bool tight) {
    PlanKnobs kn;
    if (const char* v = std::getenv("KC_SEG_CAP")) {
        kn.has_seg_cap = true;
        kn.seg_cap = std::strtoull(v, 0, 10);
    }
    if (const char* v = std::getenv("KC_SPILL_CAP")) {
        kn.has_spill_cap = true;
        kn.spill_cap = std::strtoull(v, 0, 10);
    }
    // c->win_density: windows per symbol of the batches being planned (1 for tokenized input)
    return plan_partition(c->W, syms, c->win_density, seg, g, bins1, slots, rec2, tight, kn);
}

// Partition buffers for a batch of up to `syms` symbols (lazily grown): part_plan's sizes
int ensure_part_geo(kc_ctx* c, uint64_t syms, bool seg, const PartGeo& g, PartBufs& pb, PartHist& own, uint32_t bins1,
                    uint32_t slots, uint64_t rec2) {
    const PartPlan p = part_plan(c, syms, seg, g, bins1, slots, rec2, slots > 1);
    if (!reserve_pair(own.hist1, p.n1, own.off1, p.n1 + 1) || !reserve_pair(own.hist2, p.n2, own.off2, p.n2 + 1) ||
        !own.bsum.reserve(p.nbs))
        return c->fail(KC_ERR_NOMEM, "partition histogram allocation failed");
    auto grow = [&](DevBuf<uint64_t>& buf, uint64_t need) -> int {
        if (buf.reserve(need)) return KC_OK;
        return c->fail(KC_ERR_NOMEM,
                       "partition key buffer allocation failed (" + std::to_string((size_t)need * 8) + " bytes)");
    };
    int rc = grow(c->d_keys1, p.need1);
    if (rc) return rc;
    rc = grow(c->d_keys2, p.need2);
    if (rc) return rc;
    if (p.spill_cap && (rc = grow(c->d_spill, p.spill_words))) return rc;
    pb.hist1 = own.hist1.get();
    pb.off1 = own.off1.get();
    pb.hist2 = own.hist2.get();
    pb.off2 = own.off2.get();
    pb.bsum = own.bsum.get();
    pb.spill = c->d_spill.get();
    pb.spill_cap = p.spill_cap;
    pb.keys1 = c->d_keys1.get();
    pb.keys2 = c->d_keys2.get();
    pb.nblk1 = p.nblk1;
    pb.B2 = p.B2;
    pb.cap1 = p.cap1;
    pb.cap2 = p.cap2;
    return KC_OK;
}

// the table's levels
int ensure_part(kc_ctx* c, uint64_t syms, bool seg, uint32_t bins1, uint32_t slots) {
    seg = seg && c->seg_ok;
    return ensure_part_geo(c, syms, seg, table_geo(c), c->pb, c->pb_own, bins1, slots,
                           slots > 1 ? level2_record_bytes(c->W, c->cfg.k, c->R) : 0);
}

// KC_INSERT_PATH (tests, include/kc_api.h knobs): direct | partitioned | exact forces one insert
// path for every batch; unset = chosen per batch by the cost rules below
PathKnob insert_path_knob() {
    const char* v = std::getenv("KC_INSERT_PATH");
    if (!v) return PathKnob::Auto;
    if (!std::strcmp(v, "direct")) return PathKnob::Direct;
    if (!std::strcmp(v, "partitioned")) return PathKnob::Partitioned;
    if (!std::strcmp(v, "exact")) return PathKnob::Exact;
    return PathKnob::Auto;
}

// KC_DEBUG=1: the host's decisions (partition reuse, deferred level 3) on stderr
bool debug_on() {
    const char* v = std::getenv("KC_DEBUG");
    return v && *v && *v != '0';
}

// Insert path per batch: the partitioned pipeline moves ~(4W+1)*8 bytes per window
// plus two sweeps of the table; the direct path is bound by scattered device atomics
// (~20 G/s on MI355X, i.e. ~275 bytes-equivalent per window at ~5.5 TB/s).
bool use_partitioned(const kc_ctx* c, uint64_t syms) {
    const PathKnob p = insert_path_knob();
    if (p != PathKnob::Auto) return p != PathKnob::Direct;
    const double table_bytes = (double)c->nbuckets * 128.0;
    return (double)syms * 275.0 > (double)syms * (4.0 * c->W + 1) * 8.0 + 2.0 * table_bytes;
}

// Bloom pass 1 (blocked layout): the partitioned pass moves one u64 per window three
// times plus two sweeps of the filter; the direct pass costs a scattered 64-byte line
// RMW with up to ceil(hf) device-scope atomics per window.
bool use_partitioned_bloom(const kc_ctx* c, uint64_t syms) {
    const PathKnob p = insert_path_knob();
    if (p != PathKnob::Auto) return p != PathKnob::Direct;
    const double filter_bytes = (double)bloom_words(c) * 4.0;
    return (double)syms * 275.0 > (double)syms * 5.0 * 8.0 + 2.0 * filter_bytes;
}

// the readers of the table (finish, dump, write, compact, ...): the staged work done and a
// deferred reset carried out first
int sync_for_read(kc_ctx* c) {
    JOB_OK(c);
    int rc = flush_host(c);
    if (rc) return rc;
    rc = materialize_zero(c, c->stream);  // a deferred reset is due before anyone reads the table
    if (rc) return rc;
    HIPCHK(c, hipDeviceSynchronize());
    return KC_OK;
}

// the compact representation is a snapshot of the table (kc_compact); kc_reset drops it
// The counting passes' key buffers and skew list are scratch that stays allocated between
// batches and jobs (a deferred group holds several batches' level-2 segments: C5 on one GPU,
// ~150 GB).  Before an allocation that would not fit beside them (the compact representation, a
// full dump) they are released; the next counting pass allocates them again (and cannot count
// from a Bloom pass's partitions released this way).
void make_room(kc_ctx* c, uint64_t bytes) {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess || (double)fr >= (double)bytes + (double)(1ull << 30)) return;
    if (!c->d_keys1 && !c->d_keys2 && !c->d_spill) return;
    (void)hipDeviceSynchronize();
    reset_all(c->d_keys1, c->d_keys2, c->d_spill);
    c->pb.keys1 = c->pb.keys2 = c->pb.spill = nullptr;
    c->pbf.keys1 = c->pbf.keys2 = c->pbf.spill = nullptr;
    c->reuse_img = nullptr;  // (the kept partitions are gone)
    if (debug_on()) std::fprintf(stderr, "released the partition key buffers for %.1f GB\n", bytes / 1e9);
}

void drop_compact(kc_ctx* c) {
    reset_all(c->d_cwords, c->d_csecond);
    c->cslots = c->cstarts = c->ckmers = 0;
}

extern "C" {

// ------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------
const char* kc_last_error(const kc_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int kc_create(const kc_config* cfg, kc_ctx** out) {
    if (!cfg || !out) { g_create_error = "null argument"; return KC_ERR_ARG; }
    *out = nullptr;
    if (cfg->k < 1 || cfg->k > KC_MAX_K) {
        g_create_error = "k must be in 1.." + std::to_string(KC_MAX_K);
        return KC_ERR_ARG;
    }
    static_assert(KC_MAX_K == MAX_K, "include/kc_api.h and kc_internal.h agree on the largest k");
    if (cfg->mode < 0 || cfg->mode > 2) { g_create_error = "mode must be 0, 1 or 2"; return KC_ERR_ARG; }
    if (cfg->bf_enable && (cfg->est_unique == 0 || !(cfg->fpr >= 0.001 && cfg->fpr <= 0.999))) {
        g_create_error = "bloom filter needs est_unique > 0 and 0.001 <= fpr <= 0.999";
        return KC_ERR_ARG;
    }
    kc_ctx* c = new kc_ctx();
    c->cfg = *cfg;
    if (const char* v = std::getenv("KC_STRICT_CAPACITY")) c->strict_capacity = std::atoi(v) != 0;
    c->W = words_for_k(cfg->k);
    c->S = slots_per_bucket(c->W);
    auto bail = [&](int code, const std::string& m) {
        g_create_error = m.empty() ? c->err : m;
        kc_destroy(c);
        return code;
    };
    hipError_t e = hipSetDevice(cfg->device);
    if (e != hipSuccess) return bail(KC_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
    uint64_t batch = cfg->batch_bytes;
    if (!batch) {
        // Every staged batch of the partitioned insert sweeps the table once, so batches are
        // as large as the device allows: the partition buffers take ~28 W + 4 bytes per
        // staged byte (two segmented key buffers, the skew lists, the packed stream); use ~40 % of free
        // HBM, within [256 MiB, 2 GiB] (the pinned host stage is two batches).
        size_t fr = 0, tot = 0;
        batch = kDefaultBatch;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess)
            batch = std::min<uint64_t>(2ull << 30, std::max<uint64_t>(kDefaultBatch,
                                                                       (uint64_t)(0.4 * fr) / (28 * c->W + 4)));
    }
    c->batch_bytes = round_up(batch, TILE);
    c->max_chunks = c->batch_bytes / TILE;
    if ((e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking)) != hipSuccess)
        return bail(KC_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    for (int i = 0; i < 2; i++) {  // (the pinned byte stages are allocated on first host chunk)
        if (!c->h_desc[i].reserve(c->max_chunks))
            return bail(KC_ERR_NOMEM, "pinned staging allocation failed");
        if (hipEventCreateWithFlags(&c->h_free[i], hipEventDisableTiming) != hipSuccess)
            return bail(KC_ERR_HIP, "event creation failed");
    }
    if (hipEventCreateWithFlags(&c->xev, hipEventDisableTiming) != hipSuccess)
        return bail(KC_ERR_HIP, "event creation failed");
    const uint64_t ntiles = c->batch_bytes / TILE;
    if (!c->d_pk.reserve((c->batch_bytes + c->max_chunks) / 32 + 4) ||
        !c->d_bk.reserve((c->batch_bytes + c->max_chunks) / 32 + 4) || !c->d_tiles.reserve(ntiles) ||
        !c->d_touts.reserve(ntiles) || !c->d_tblk.reserve(ntiles / 1024 + 2) || !c->d_chunks.reserve(c->max_chunks) ||
        !c->d_ctr.reserve(1) || !c->d_sum.reserve(2 * CHECKSUM_SLOTS))
        return bail(KC_ERR_NOMEM, "device staging allocation failed");
    if (hipMemsetAsync(c->d_ctr, 0, sizeof(DevCounters), c->stream) != hipSuccess)
        return bail(KC_ERR_HIP, "memset failed");
    if (cfg->bf_enable) {
        bloom_sizes(cfg->est_unique, cfg->fpr, &c->bf_bits, &c->nh, &c->nh_gate);
        if (c->nh > MAX_NH) return bail(KC_ERR_ARG, "too many Bloom hash functions");
        if (bloom_blocks(c->bf_bits) > (1ULL << 32)) return bail(KC_ERR_ARG, "Bloom filter too large (-u)");
        const char* lay = std::getenv("KC_BLOOM_LAYOUT");
        c->bloom_blocked = !(lay && !std::strcmp(lay, "reference"));
        const uint64_t words = bloom_words(c);
        if (!c->d_bloom.reserve(words))
            return bail(KC_ERR_NOMEM, "Bloom filter allocation failed");
        if (hipMemsetAsync(c->d_bloom, 0, words * 4, c->stream) != hipSuccess) return bail(KC_ERR_HIP, "memset");
        c->bloom_fresh = true;
        if (c->bloom_blocked) {
            // filter regions of up to BF_BLOCKS_PER_REGION (1024) blocks = 64 KiB, F1 x F2 as
            // for the table (all powers of two here)
            const uint64_t nb = bloom_blocks(c->bf_bits);
            const uint64_t R = std::max<uint64_t>(1, nb / BF_BLOCKS_PER_REGION);
            int rbits = 0;
            while ((1ULL << rbits) < R) rbits++;
            const int f1bits = std::min(10, (rbits + 1) / 2);
            c->bgeo.R = R;
            c->bgeo.f2bits = rbits - f1bits;
            c->bgeo.F2 = 1u << c->bgeo.f2bits;
            c->bgeo.F1 = (uint32_t)(R >> c->bgeo.f2bits);
            c->bgeo.W = 1;
            // partition reuse: fine bins for a table of up to 2 * est_unique slots (the table
            // of the counting pass holds 2 * new_in_second <= about 2 * -u), never coarser than
            // the filter regions, and as fine as level 1 (two workgroups per CU), level 2 and
            // k_b3 (segments per filter region) allow
            {
                uint64_t want = std::max<uint64_t>(2 * cfg->est_unique, 64);
                want += want / 4;
                const uint64_t regions = std::max<uint64_t>(1, ((want + c->S - 1) / c->S + BPR - 1) / BPR);
                int fb = rbits, f1 = 0;
                while ((1ULL << fb) < regions) fb++;
                // (wide keys run one level-1 workgroup per CU anyway)
                const size_t p1_cap = p1_lds_bytes(c->W, 1) <= 80 * 1024 ? 80 * 1024 : 160 * 1024;
                for (; fb >= rbits; fb--) {
                    f1 = std::min(fb, std::min(8, (fb + 1) / 2 + 1));
                    while (f1 > 0 && p1_lds_bytes(c->W, 1u << f1) > p1_cap) f1--;
                    const uint32_t F2 = 1u << (fb - f1), F1 = 1u << f1;
                    const uint32_t B2 = std::max<uint32_t>(1, std::min<uint32_t>(64, 2048 / F1));
                    // (budgeted at 32 bytes per level-2 bin, as before the scatter's bins
                    // took 24: the finer bins that now fit, F2 = 1024 at C3's -u, measured
                    // slower, 29.0 vs 31-32 G k-mers/s, profiles/r02_v15_bench.json)
                    if (p2f_lds_bytes(c->W, F2, 2048 / B2 + 1) + (size_t)F2 * 8 <= 160 * 1024 &&
                        (1ULL << (fb - rbits)) * B2 <= MAX_SEG_GROUP)
                        break;
                }
                if (fb >= rbits) {
                    c->fgeo_max_R = 1ULL << fb;
                    // the job starts at no more than 2^16 fine bins: -u usually overstates the
                    // k-mers that pass the gate (C3: -u 4e8 for 50 M), and level 2's 256-bin
                    // scatter of C2's table is the fastest shape
                    while (fb > rbits && (1ULL << fb) > (1ULL << 16)) fb--;
                    f1 = std::min(fb, std::min(8, (fb + 1) / 2 + 1));
                    while (f1 > 0 && p1_lds_bytes(c->W, 1u << f1) > p1_cap) f1--;
                    c->fgeo.R = 1ULL << fb;
                    c->fgeo.f2bits = fb - f1;
                    c->fgeo.F2 = 1u << c->fgeo.f2bits;
                    c->fgeo.F1 = 1u << f1;
                    c->fgeo.W = c->W;
                }
            }
        }
    } else {
        int rc = alloc_table(c, cfg->table_slots);
        if (rc) return bail(rc, "");
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) return bail(KC_ERR_HIP, "stream sync failed");
    *out = c;
    return KC_OK;
}

void kc_destroy(kc_ctx* c) {
    if (!c) return;
    if (c->stream) hipStreamSynchronize(c->stream);
    for (auto e : c->h_free)
        if (e) hipEventDestroy(e);
    if (c->xev) hipEventDestroy(c->xev);
    if (c->seq_ev) hipEventDestroy(c->seq_ev);
    for (auto e : c->aev)
        if (e) hipEventDestroy(e);
    if (c->aux) hipStreamDestroy(c->aux);
    for (auto e : c->ev_pool) hipEventDestroy(e);
    for (auto& ev : c->ev_pending)
        for (auto e : ev)
            if (e) hipEventDestroy(e);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

int kc_size_table(kc_ctx* c, uint64_t slots) {
    if (!c) return KC_ERR_ARG;
    JOB_OK(c);
    if (c->cfg.bf_enable) return c->fail(KC_ERR_STATE, "a Bloom job sizes its table from new_in_second");
    if (!c->table_fresh || c->n_chunks) return c->fail(KC_ERR_STATE, "kc_size_table: the job has counted already");
    int rc = flush_host(c);
    if (rc) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipDeviceSynchronize());  // (the previous job's passes may still read the table)
    const uint64_t phys = slots ? slots : c->cfg.table_slots;
    // a table well below its allocation gives the memory back (the deferred level 3 sizes its
    // groups from free HBM); the same size job after job keeps its allocation
    const uint64_t want = std::max<uint64_t>(phys, 64) + std::max<uint64_t>(phys, 64) / 4;
    const uint64_t bytes = (want + c->S - 1) / c->S * (BUCKET_WORDS * 8) + (uint64_t)BPR * BUCKET_WORDS * 8;
    if (c->d_table && bytes * 4 < c->d_table.capacity() * 8 * 3) c->d_table.reset();
    return alloc_table(c, c->cfg.table_slots, 0, phys);  // (ensure_part re-plans the levels per batch)
}

// (a deferred reset stays deferred: the next fresh pass writes every region anyway -- the
// sharded merge empties the local table and syncs every step)
int kc_sync(kc_ctx* c) {
    if (!c) return KC_ERR_ARG;
    int rc = flush_host(c);
    if (rc) return rc;
    HIPCHK(c, hipDeviceSynchronize());
    return KC_OK;
}

int kc_finish(kc_ctx* c, kc_stats* st) {
    if (!c) return KC_ERR_ARG;
    int rc = sync_for_read(c);
    if (rc) return rc;
    DevCounters h;
    HIPCHK(c, hipMemcpy(&h, c->d_ctr, sizeof(h), hipMemcpyDeviceToHost));
    if (st) {
        std::memset(st, 0, sizeof(*st));
        st->windows = h.windows;
        st->bf_windows = h.bf_windows;
        st->inserted = h.inserted;
        st->table_slots = c->nbuckets * c->S;
        st->bf_bits = c->bf_bits;
        st->new_in_first = h.new_in_first;
        st->new_in_second = h.new_in_second;
        st->failed_in_first = h.failed_in_first;
        st->chunks = c->n_chunks;
        st->part_fallbacks = h.part_fallbacks;
        st->spilled = h.spilled;
        st->heavy_records = h.heavy;
        st->reused_passes = c->reuse_hits;
        st->reuse_level = (uint64_t)c->reuse_last_level;
        st->route_counts_kept = c->route_counts_kept;
        st->deferred_level3 = c->defer_groups;
        st->bytes = c->n_bytes;
        // occupied slots
        if (c->nbuckets) {
            HIPCHK(c, hipMemsetAsync(&c->d_ctr->occupied, 0, 8, c->stream));
            HIPCHK(c, hipMemsetAsync(&c->d_ctr->dump_n, 0, 8, c->stream));
            TableView tv = table_view(c);
            HIPCHK(c, launch_dump(tv, c->cfg.mode == 0 ? 0 : 1, ~0ULL, nullptr, c->d_ctr, c->stream));
            unsigned long long occ = 0;
            HIPCHK(c, hipMemcpyAsync(&occ, &c->d_ctr->occupied, 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            st->distinct = occ;
        }
    }
    if (h.invalid)
        return c->fail(KC_ERR_ARG, std::to_string(h.invalid) + " keys passed to kc_insert_keys_device were not table keys "
                                   "(word 0 == 0) and were skipped");
    if (h.overflow) return c->fail(KC_ERR_TABLE_FULL, "Hash table is full (" + std::to_string(h.overflow) +
                                                           " k-mers could not be inserted)");
    if (c->strict_capacity && c->nbuckets) {  // the reference's table: next_prime3mod4(min slots)
        const uint64_t cap = kc_table_size_reference(c->min_slots);
        TableView tv = table_view(c);
        HIPCHK(c, hipMemsetAsync(&c->d_ctr->occupied, 0, 8, c->stream));
        HIPCHK(c, launch_dump(tv, c->cfg.mode == 0 ? 0 : 1, ~0ULL, nullptr, c->d_ctr, c->stream));
        unsigned long long occ = 0;
        HIPCHK(c, hipMemcpyAsync(&occ, &c->d_ctr->occupied, 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (occ > cap)
            return c->fail(KC_ERR_TABLE_FULL, "Hash table is full (" + std::to_string(occ) + " distinct k-mers, the "
                                              "reference's table holds " + std::to_string(cap) + ")");
    }
    return KC_OK;
}

int kc_clear_table(kc_ctx* c) {
    if (!c) return KC_ERR_ARG;
    if (!c->nbuckets) return c->fail(KC_ERR_STATE, "no table");
    c->table_zero_pending = true;  // deferred: see materialize_zero
    c->table_fresh = true;
    c->own_valid = false;
    return KC_OK;
}

int kc_reset(kc_ctx* c) {
    if (!c) return KC_ERR_ARG;
    int rc = kc_sync(c);
    if (rc) return rc;
    if (c->d_table) {
        c->table_zero_pending = true;  // deferred: see materialize_zero
        c->table_fresh = true;
        c->own_valid = false;
    }
    if (c->d_bloom) {
        HIPCHK(c, hipMemsetAsync(c->d_bloom, 0, bloom_words(c) * 4, c->stream));
        c->bloom_fresh = true;
        if (c->bloom_final) {  // back to the Bloom pass: the table is sized again after it
            // (its allocation is kept for reuse; ensure_part_geo re-sizes the histograms)
            c->nbuckets = 0;
            c->bloom_final = false;
        }
    }
    HIPCHK(c, hipMemsetAsync(c->d_ctr, 0, sizeof(DevCounters), c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->n_chunks = c->n_bytes = 0;
    c->bloom_batches = 0;
    drop_compact(c);
    c->reuse_kept = c->reuse_ok = false;
    c->reuse_level = 0;
    if (c->fgeo_next_R && c->fgeo_next_R != c->fgeo.R && c->fgeo_next_R <= c->fgeo_max_R) {
        int fb = 0, f1 = 0;
        while ((1ULL << fb) < c->fgeo_next_R) fb++;
        while ((1u << f1) < c->fgeo.F1) f1++;
        c->fgeo.R = 1ULL << fb;
        c->fgeo.f2bits = fb - f1;
        c->fgeo.F2 = 1u << c->fgeo.f2bits;
    }
    c->fgeo_next_R = 0;
    c->reuse_hits = 0;
    c->reuse_last_level = 0;
    c->route_counts_kept = 0;
    c->defer_groups = 0;
    c->defer_n = 0;
    c->skew_prev = c->heavy_prev = 0;
    c->defer_on = c->defer_last = false;
    c->broken.clear();
    c->kept_valid = false;
    return KC_OK;
}

int kc_profile(kc_ctx* c, int enable) {
    if (!c) return KC_ERR_ARG;
    c->profiling = enable != 0;
    return KC_OK;
}

int kc_get_timing(kc_ctx* c, kc_timing* t) {
    if (!c || !t) return KC_ERR_ARG;
    int rc = kc_sync(c);
    if (rc) return rc;
    for (auto& ev : c->ev_pending) {
        float a = 0, b = 0, d = 0;
        if (ev[0]) {  // a full batch: {start, gather, tokenize, count/route}
            HIPCHK(c, hipEventElapsedTime(&a, ev[0], ev[1]));
            HIPCHK(c, hipEventElapsedTime(&b, ev[1], ev[2]));
            c->timing.launches++;
        }
        HIPCHK(c, hipEventElapsedTime(&d, ev[2], ev[3]));  // insert of received keys: {-, -, start, end}
        c->timing.gather_ms += a;
        c->timing.tokenize_ms += b;
        c->timing.count_ms += d;
        for (auto e : ev)
            if (e) c->ev_pool.push_back(e);
    }
    c->ev_pending.clear();
    unsigned long long sl = 0;
    HIPCHK(c, hipMemcpy(&sl, &c->d_ctr->stream_len, 8, hipMemcpyDeviceToHost));
    c->timing.symbols = sl;  // symbols of the LAST batch (exact for single-batch steps)
    *t = c->timing;
    c->timing = kc_timing{};
    return KC_OK;
}

int kc_key_words(const kc_ctx* c) { return c ? c->W : 0; }

void kc_free(void* p) { std::free(p); }

uint64_t kc_table_size_reference(uint64_t at_least) {  // next_prime3mod4, functions_math.cpp:53-96
    if (at_least <= 2) return 2;
    uint64_t p = at_least % 2 == 0 ? at_least + 1 : at_least;
    for (;; p += 2) {
        bool prime = true;
        for (uint64_t d = 3; d * d <= p; d += 2)
            if (p % d == 0) { prime = false; break; }
        if (prime && p % 4 == 3) return p;
    }
}

int kc_bloom_info(kc_ctx* c, uint64_t* n_words, uint64_t* bits, int* nh, int* nh_gate, int* layout) {
    if (!c) return KC_ERR_ARG;
    if (!c->d_bloom) return c->fail(KC_ERR_STATE, "no Bloom filter");
    if (n_words) *n_words = bloom_words(c);
    if (bits) *bits = c->bf_bits;
    if (nh) *nh = c->nh;
    if (nh_gate) *nh_gate = c->nh_gate;
    if (layout) *layout = c->bloom_blocked;
    return KC_OK;
}

int kc_bloom_read(kc_ctx* c, uint32_t* words, uint64_t n) {
    if (!c || (!words && n)) return KC_ERR_ARG;
    if (!c->d_bloom) return c->fail(KC_ERR_STATE, "no Bloom filter");
    if (n > bloom_words(c)) return c->fail(KC_ERR_ARG, "more words than the filter holds");
    int rc = kc_sync(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(words, c->d_bloom, n * 4, hipMemcpyDeviceToHost));
    return KC_OK;
}

int kc_bloom_write(kc_ctx* c, const uint32_t* words, uint64_t n) {
    if (!c || (!words && n)) return KC_ERR_ARG;
    if (!c->d_bloom) return c->fail(KC_ERR_STATE, "no Bloom filter");
    if (n > bloom_words(c)) return c->fail(KC_ERR_ARG, "more words than the filter holds");
    int rc = kc_sync(c);
    if (rc) return rc;
    HIPCHK(c, hipMemcpy(c->d_bloom, words, n * 4, hipMemcpyHostToDevice));
    c->bloom_fresh = false;
    return KC_OK;
}

}  // extern "C"
