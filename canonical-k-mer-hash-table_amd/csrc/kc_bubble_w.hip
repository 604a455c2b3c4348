// kc_bubble_w.hip -- bubble popping's anchor and verdict kernels (kc_bubble_impl.h) for ONE key
// width: compiled once per W with -DKC_W=1..15, like kc_clean_w.hip.
#ifndef KC_W
#error "compile with -DKC_W=<key words>"
#endif
#include "kc_internal.h"
#include "kc_bubble_impl.h"

namespace kc {
template struct BubbleOps<KC_W>;
}  // namespace kc
