// translation unit: the search-free null-space elimination (k_backward_ns), every row of CE_NS_VARIANTS for each mode of one kind
//   -DCE_NS_QP=0 linear objective (adjoint, forward derivative, refinement), 1 quadratic objective inside the elimination (forward derivative, refinement)
//   -DCE_NS_QP=0 -DCE_NS_TRI=1 linear objective with exponential / power triples (forward derivative, refinement)
//   (one object file per kind: csrc/Makefile)
#include "ce_tu_prologue.h"
#include "ce_variants.h"
namespace {
#include "ce_backward_ns.h"
}  // namespace

#ifndef CE_NS_QP
#error "compile with -DCE_NS_QP=0|1"
#endif
#ifndef CE_NS_TRI
#define CE_NS_TRI 0
#endif
#if CE_NS_QP != 0 && CE_NS_TRI != 0
#error "no kind has both a quadratic objective and triples"
#endif
// Y(FWD, REF, QP, TRI, the mode's argument struct): the instantiations of this object's kind
#if CE_NS_TRI != 0
#define NS_MODES(Y) Y(true, false, false, true, NsJvpTri) Y(true, true, false, true, NsRefineTri)
#define NS_SETATTR ce_setattr_ns_tri
#elif CE_NS_QP == 0
#define NS_MODES(Y) Y(false, false, false, false, NsNoJvp) Y(true, false, false, false, NsJvp) Y(true, true, false, false, NsRefine)
#define NS_SETATTR ce_setattr_ns
#else
#define NS_MODES(Y) Y(true, false, true, false, NsJvpQp) Y(true, true, true, false, NsRefineQp)
#define NS_SETATTR ce_setattr_ns_qp
#endif

namespace {
// (a mode reads the fields of CeBwdArgs it needs; the host leaves the others null)
template <bool FWD, bool REF, bool QP, bool TRI, class Args>
int launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const Args &w0) {
    Args w = w0;
    if constexpr (std::is_same<Args, NsNoJvp>::value) w.dA_factors = a.dA_factors;          // (the single-cotangent adjoint's factor mode: CeBwdArgs states it, the kernel reads its mode struct)
    switch (variant) {
#define X(V, NTILE, NTHR) case V: hipLaunchKernelGGL((k_backward_ns<NTILE, NTHR, FWD, REF, QP, TRI>), dim3(B), dim3(NTHR), lds, st, a.T, a.Abm, a.x, a.y, a.s, a.dx, a.dy, a.dA, a.dq, a.sdqk, a.sdqb, a.adj, a.fix, w); return 0;
        CE_NS_VARIANTS(X)
#undef X
    default: return -1;
    }
}
template <bool FWD, bool REF, bool QP, bool TRI>
hipError_t setattr_ns(int bytes) {
#define X(V, NTILE, NTHR) { const hipError_t e_ = ce_set_max_lds(&k_backward_ns<NTILE, NTHR, FWD, REF, QP, TRI>, bytes); if (e_ != hipSuccess) return e_; }
    CE_NS_VARIANTS(X)
#undef X
    return hipSuccess;
}
}  // namespace

#define Y(FWD, REF, QP, TRI, Args) int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const Args &w) { return launch_ns<FWD, REF, QP, TRI>(variant, B, lds, st, a, w); }
NS_MODES(Y)
#undef Y
hipError_t NS_SETATTR(int bytes) {
#define Y(FWD, REF, QP, TRI, Args) { const hipError_t e_ = setattr_ns<FWD, REF, QP, TRI>(bytes); if (e_ != hipSuccess) return e_; }
    NS_MODES(Y)
#undef Y
    return hipSuccess;
}
