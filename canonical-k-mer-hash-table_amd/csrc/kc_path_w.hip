// kc_path_w.hip -- the read paths' locate kernel (kc_path_impl.h) for ONE key width: compiled once
// per W with -DKC_W=1..15, like kc_seq_w.hip.
#ifndef KC_W
#error "compile with -DKC_W=<key words>"
#endif
#include "kc_internal.h"
#include "kc_path_impl.h"

namespace kc {
template struct PathOps<KC_W>;
}  // namespace kc
