// kc_query_w.hip -- the table-query kernels (kc_query_impl.h) for ONE key width: compiled once
// per W with -DKC_W=1..15, like kc_compact_w.hip.  -DKC_QUERY_TPK builds the one- and two-word
// lookups in the thread-per-key form as well (the A/B of tools/lookup_probe.py).
#ifndef KC_W
#error "compile with -DKC_W=<key words>"
#endif
#include "kc_internal.h"
#include "kc_query_impl.h"

namespace kc {
template struct QueryOps<KC_W>;
}  // namespace kc
