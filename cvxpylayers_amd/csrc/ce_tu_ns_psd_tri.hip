// translation unit: the search-free null-space elimination with PSD blocks AND exponential / power triples beside the plain cones
// (k_backward_ns<..., FWD, REF or not, ..., TRI, ..., PSD>), every row of CE_NS_VARIANTS for the forward derivative (ce_jvp_psd_tri) and the refinement step
// (ce_refine_psd_tri).  An object of its own (csrc/Makefile ns_psd_tri.o) with its own LDS attribute setter, beside ce_tu_ns_psd.hip, whose instantiations stay.
#include "ce_tu_prologue.h"
#include "ce_variants.h"
namespace {
#include "ce_backward_ns.h"
}  // namespace

namespace {
template <bool REF, class Args>
int launch_ns_psd_tri(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const Args &w) {
    switch (variant) {
#define X(V, NTILE, NTHR) case V: hipLaunchKernelGGL((k_backward_ns<NTILE, NTHR, true, REF, false, true, false, true>), dim3(B), dim3(NTHR), lds, st, a.T, a.Abm, a.x, a.y, a.s, a.dx, a.dy, a.dA, a.dq, a.sdqk, a.sdqb, a.adj, a.fix, w); return 0;
        CE_NS_VARIANTS(X)
#undef X
    default: return -1;
    }
}
template <bool REF>
hipError_t setattr_ns_psd_tri(int bytes) {
#define X(V, NTILE, NTHR) { const hipError_t e_ = ce_set_max_lds(&k_backward_ns<NTILE, NTHR, true, REF, false, true, false, true>, bytes); if (e_ != hipSuccess) return e_; }
    CE_NS_VARIANTS(X)
#undef X
    return hipSuccess;
}
}  // namespace

int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsJvpPsdTri &w) { return launch_ns_psd_tri<false>(variant, B, lds, st, a, w); }
int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsRefinePsdTri &w) { return launch_ns_psd_tri<true>(variant, B, lds, st, a, w); }
hipError_t ce_setattr_ns_psd_tri(int bytes) {
    { const hipError_t e_ = setattr_ns_psd_tri<false>(bytes); if (e_ != hipSuccess) return e_; }
    return setattr_ns_psd_tri<true>(bytes);
}
