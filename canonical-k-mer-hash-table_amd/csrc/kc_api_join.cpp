// kc_api_join.cpp -- table algebra (include/kc_api.h kc_table_op*): intersect, subtract and union
// two counted tables in HBM into a third, and the statistics that compare them.  Kernel:
// kc_join_impl.h (one fused sweep / probe / insert launch, a second one for the unions).
#include "kc_ctx.h"

#pragma GCC visibility push(hidden)

static_assert(sizeof(kc_op_desc) == 24 && sizeof(kc_op_stats) == 40, "include/kc_api.h states these sizes");

static bool op_is_union(int op) { return op == KC_OP_UNION_SUM || op == KC_OP_UNION_MAX; }

// what both forms check before they touch the device; err receives the message
static int op_check(kc_ctx* err, kc_ctx* dst, kc_ctx* a, kc_ctx* b, const kc_op_desc* op) {
    if (dst && (dst == a || dst == b)) return err->fail(KC_ERR_ARG, "kc_table_op: dst must not be an operand");
    for (kc_ctx* x : {dst, b})
        if (x && (x->cfg.k != a->cfg.k || x->cfg.device != a->cfg.device))
            return err->fail(KC_ERR_ARG, "kc_table_op: the contexts must have the same k and device");
    if (op->op < KC_OP_INTERSECT_MIN || op->op > KC_OP_UNION_MAX) return err->fail(KC_ERR_ARG, "kc_table_op: unknown op");
    if (op->reserved) return err->fail(KC_ERR_ARG, "kc_table_op: reserved must be 0");
    if ((op->a_max && op->a_min > op->a_max) || (op->b_max && op->b_min > op->b_max))
        return err->fail(KC_ERR_ARG, "kc_table_op: a range's min is above its max");
    for (kc_ctx* x : {dst, a, b}) {
        if (!x) continue;
        if (!x->broken.empty()) return err->fail(KC_ERR_STATE, x->broken + " (kc_reset first)");
        if (!x->nbuckets) return err->fail(KC_ERR_STATE, "no table (kc_bloom_finalize must precede a table operation)");
    }
    return KC_OK;
}

#pragma GCC visibility pop

extern "C" {

int kc_table_op_device(kc_ctx* dst, kc_ctx* a, kc_ctx* b, const kc_op_desc* op, kc_op_stats* dev_stats, void* sp) {
    kc_ctx* err = dst ? dst : a;
    if (!a || !b || !op) return err ? err->fail(KC_ERR_ARG, "kc_table_op: null operand or descriptor") : KC_ERR_ARG;
    int rc = op_check(err, dst, a, b, op);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)sp;
    for (kc_ctx* x : {dst, a, b != a ? b : nullptr})
        if (x && (rc = route_rc(err, x, flush_host(x)))) return rc;
    // one scope per distinct context: s waits for each one's stream, each then waits for s
    StreamScope on_a(a, s), on_b(b, s);  // (a == b: on_b is never joined)
    if ((rc = route_rc(err, a, on_a.join()))) return rc;
    if (b != a && (rc = route_rc(err, b, on_b.join()))) return rc;
    // an emptied operand holds nothing (and its memory is not read before it is zeroed)
    if ((rc = route_rc(err, a, materialize_zero(a, s)))) return rc;
    if ((rc = route_rc(err, b, materialize_zero(b, s)))) return rc;
    unsigned long long* st = reinterpret_cast<unsigned long long*>(dev_stats);
    if (st) HIPCHK(err, hipMemsetAsync(st, 0, sizeof(kc_op_stats), s));
    const uint32_t a_min = op->a_min ? op->a_min : 1, b_min = op->b_min ? op->b_min : 1;
    const int ma = a->cfg.mode == 0 ? 0 : 1, mb = b->cfg.mode == 0 ? 0 : 1;
    auto work = [&]() -> int {
        const TableView ta = table_view(a), tb = table_view(b), td = dst ? table_view(dst) : TableView{};
        DevCounters* ctr = dst ? dst->d_ctr.get() : nullptr;
        HIPCHK(err, launch_join(ta, tb, td, ma, mb, a_min, op->a_max, b_min, op->b_max, op->op, 0, ctr, st, s));
        if (op_is_union(op->op))  // the keys of b that a lacks
            HIPCHK(err, launch_join(tb, ta, td, mb, ma, b_min, op->b_max, a_min, op->a_max, op->op, 1, ctr, st, s));
        return KC_OK;
    };
    rc = write_dst(dst, s, work);
    if (rc) return rc;
    if ((rc = route_rc(err, a, on_a.finish()))) return rc;
    return route_rc(err, b, on_b.finish());
}

int kc_table_op(kc_ctx* dst, kc_ctx* a, kc_ctx* b, const kc_op_desc* op, kc_op_stats* stats) {
    kc_ctx* err = dst ? dst : a;
    if (!a || !b || !op) return err ? err->fail(KC_ERR_ARG, "kc_table_op: null operand or descriptor") : KC_ERR_ARG;
    int rc = op_check(err, dst, a, b, op);
    if (rc) return rc;
    return stats_host_form(err, "kc_table_op", stats,
                           [&](kc_op_stats* d, hipStream_t s) { return kc_table_op_device(dst, a, b, op, d, s); });
}

}  // extern "C"
