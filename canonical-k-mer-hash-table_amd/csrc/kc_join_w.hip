// kc_join_w.hip -- the table-algebra kernel (kc_join_impl.h) for ONE key width: compiled once
// per W with -DKC_W=1..15, like kc_query_w.hip.
#ifndef KC_W
#error "compile with -DKC_W=<key words>"
#endif
#include "kc_internal.h"
#include "kc_join_impl.h"

namespace kc {
template struct JoinOps<KC_W>;
}  // namespace kc
