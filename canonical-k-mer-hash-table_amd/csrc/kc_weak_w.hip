// kc_weak_w.hip -- weak-link removal's verdict kernel (kc_weak_impl.h) for ONE key width: compiled
// once per W with -DKC_W=1..15, like kc_bubble_w.hip.
#ifndef KC_W
#error "compile with -DKC_W=<key words>"
#endif
#include "kc_internal.h"
#include "kc_weak_impl.h"

namespace kc {
template struct WeakOps<KC_W>;
}  // namespace kc
