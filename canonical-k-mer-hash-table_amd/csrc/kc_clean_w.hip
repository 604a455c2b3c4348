// kc_clean_w.hip -- the graph cleaning's copy kernel (kc_clean_impl.h) for ONE key width: compiled
// once per W with -DKC_W=1..15, like kc_join_w.hip.
#ifndef KC_W
#error "compile with -DKC_W=<key words>"
#endif
#include "kc_internal.h"
#include "kc_clean_impl.h"

namespace kc {
template struct CleanOps<KC_W>;
}  // namespace kc
