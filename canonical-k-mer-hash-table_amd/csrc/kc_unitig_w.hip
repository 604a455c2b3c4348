// kc_unitig_w.hip -- the unitig kernels that touch a key (kc_unitig_impl.h) for ONE key width:
// compiled once per W with -DKC_W=1..15, like kc_graph_w.hip.
#ifndef KC_W
#error "compile with -DKC_W=<key words>"
#endif
#include "kc_internal.h"
#include "kc_unitig_impl.h"

namespace kc {
template struct UnitigOps<KC_W>;
}  // namespace kc
