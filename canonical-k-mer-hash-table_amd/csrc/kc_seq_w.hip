// kc_seq_w.hip -- the per-position count kernel (kc_seq_impl.h) for ONE key width: compiled once
// per W with -DKC_W=1..15, like kc_query_w.hip.
#ifndef KC_W
#error "compile with -DKC_W=<key words>"
#endif
#include "kc_internal.h"
#include "kc_seq_impl.h"

namespace kc {
template struct SeqOps<KC_W>;
}  // namespace kc
