// translation unit: the search-free elimination with a quadratic objective (k_backward_ns<..., FWD, REF or not, QP = true>): forward derivative and
// Newton refinement of native-QP templates.  Every row of CE_NS_VARIANTS; the linear-objective instantiations live in ce_tu_bwd_rt.hip.
#include "ce_tu_prologue.h"
#include "ce_variants.h"
namespace {
#include "ce_common.h"
#include "ce_expcone.h"
#include "ce_forward_rt.h"
#include "ce_forward_v2.h"
#include "ce_global_mv.h"
#include "ce_backward.h"
#include "ce_backward_rt.h"
#include "ce_backward_ns.h"
}  // namespace

int ce_launch_fwd_ns_qp(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsJvpQp &w) {
    switch (variant) {
#define X(V, NTILE, NTHR) case V: hipLaunchKernelGGL((k_backward_ns<NTILE, NTHR, true, false, true>), dim3(B), dim3(NTHR), lds, st, a.T, a.Abm, a.x, a.y, a.s, nullptr, nullptr, nullptr, nullptr, 0L, 0L, a.adj, nullptr, w); return 0;
        CE_NS_VARIANTS(X)
#undef X
    default: return -1;
    }
}
int ce_launch_refine_ns_qp(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsRefineQp &w) {
    switch (variant) {
#define X(V, NTILE, NTHR) case V: hipLaunchKernelGGL((k_backward_ns<NTILE, NTHR, true, true, true>), dim3(B), dim3(NTHR), lds, st, a.T, a.Abm, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0L, 0L, nullptr, nullptr, w); return 0;
        CE_NS_VARIANTS(X)
#undef X
    default: return -1;
    }
}
hipError_t ce_setattr_bwd_ns_qp(int bytes) {
#define X(V, NTILE, NTHR) { hipError_t e_ = ce_set_max_lds(&k_backward_ns<NTILE, NTHR, true, false, true>, bytes); if (e_ != hipSuccess) return e_; \
                            e_ = ce_set_max_lds(&k_backward_ns<NTILE, NTHR, true, true, true>, bytes); if (e_ != hipSuccess) return e_; }
    CE_NS_VARIANTS(X)
#undef X
    return hipSuccess;
}
