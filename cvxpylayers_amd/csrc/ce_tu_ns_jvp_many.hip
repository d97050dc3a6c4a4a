// translation unit: the many-tangent mode of the search-free forward derivative (k_backward_ns<..., FWD, ..., MANY>), every row of the kind's variant list
//   (CE_NS_QP=0: linear objective, CE_NS_QP=1: P inside; one object per kind beside those of ce_tu_ns.hip and ce_tu_ns_many.hip: csrc/Makefile)
#include "ce_tu_prologue.h"
#include "ce_variants.h"
namespace {
#include "ce_backward_ns.h"
}  // namespace

#if CE_NS_QP
#define NS_ROWS CE_NS_VARIANTS
#define NS_ARG NsJvpQpMany
#define NS_SETATTR ce_setattr_ns_jvp_qp_many
#else
#define NS_ROWS CE_NS_VARIANTS
#define NS_ARG NsJvpMany
#define NS_SETATTR ce_setattr_ns_jvp_many
#endif

int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NS_ARG &w) {
    switch (variant) {
#define X(V, NTILE, NTHR) case V: hipLaunchKernelGGL((k_backward_ns<NTILE, NTHR, true, false, CE_NS_QP != 0, false, true>), dim3(B), dim3(NTHR), lds, st, a.T, a.Abm, a.x, a.y, a.s, a.dx, a.dy, a.dA, a.dq, a.sdqk, a.sdqb, a.adj, a.fix, w); return 0;
        NS_ROWS(X)
#undef X
    default: return -1;
    }
}
hipError_t NS_SETATTR(int bytes) {
#define X(V, NTILE, NTHR) { const hipError_t e_ = ce_set_max_lds(&k_backward_ns<NTILE, NTHR, true, false, CE_NS_QP != 0, false, true>, bytes); if (e_ != hipSuccess) return e_; }
    NS_ROWS(X)
#undef X
    return hipSuccess;
}
