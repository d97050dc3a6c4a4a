// translation unit: the search-free null-space elimination (k_backward_ns), every row of CE_NS_VARIANTS for each mode of one kind
//   -DCE_NS_QP=0 linear objective (adjoint, forward derivative, refinement), 1 quadratic objective inside the elimination (forward derivative, refinement)
//   (one object file per kind: csrc/Makefile)
#include "ce_tu_prologue.h"
#include "ce_variants.h"
namespace {
#include "ce_backward_ns.h"
}  // namespace

#ifndef CE_NS_QP
#error "compile with -DCE_NS_QP=0|1"
#endif
// Y(FWD, REF, QP, the mode's argument struct): the instantiations of this object's kind
#if CE_NS_QP == 0
#define NS_MODES(Y) Y(false, false, false, NsNoJvp) Y(true, false, false, NsJvp) Y(true, true, false, NsRefine)
#define NS_SETATTR ce_setattr_ns
#else
#define NS_MODES(Y) Y(true, false, true, NsJvpQp) Y(true, true, true, NsRefineQp)
#define NS_SETATTR ce_setattr_ns_qp
#endif

namespace {
// (a mode reads the fields of CeBwdArgs it needs; the host leaves the others null)
template <bool FWD, bool REF, bool QP, class Args>
int launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const Args &w) {
    switch (variant) {
#define X(V, NTILE, NTHR) case V: hipLaunchKernelGGL((k_backward_ns<NTILE, NTHR, FWD, REF, QP>), dim3(B), dim3(NTHR), lds, st, a.T, a.Abm, a.x, a.y, a.s, a.dx, a.dy, a.dA, a.dq, a.sdqk, a.sdqb, a.adj, a.fix, w); return 0;
        CE_NS_VARIANTS(X)
#undef X
    default: return -1;
    }
}
template <bool FWD, bool REF, bool QP>
hipError_t setattr_ns(int bytes) {
#define X(V, NTILE, NTHR) { const hipError_t e_ = ce_set_max_lds(&k_backward_ns<NTILE, NTHR, FWD, REF, QP>, bytes); if (e_ != hipSuccess) return e_; }
    CE_NS_VARIANTS(X)
#undef X
    return hipSuccess;
}
}  // namespace

#define Y(FWD, REF, QP, Args) int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const Args &w) { return launch_ns<FWD, REF, QP>(variant, B, lds, st, a, w); }
NS_MODES(Y)
#undef Y
hipError_t NS_SETATTR(int bytes) {
#define Y(FWD, REF, QP, Args) { const hipError_t e_ = setattr_ns<FWD, REF, QP>(bytes); if (e_ != hipSuccess) return e_; }
    NS_MODES(Y)
#undef Y
    return hipSuccess;
}
