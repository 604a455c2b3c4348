// kc_correct_w.hip -- the try kernel of the read correction (kc_correct_impl.h) for ONE key width:
// compiled once per W with -DKC_W=1..15, like kc_seq_w.hip.
#ifndef KC_W
#error "compile with -DKC_W=<key words>"
#endif
#include "kc_internal.h"
#include "kc_correct_impl.h"

namespace kc {
template struct CorrectOps<KC_W>;
}  // namespace kc
