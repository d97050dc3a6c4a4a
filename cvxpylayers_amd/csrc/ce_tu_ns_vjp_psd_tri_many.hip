// translation unit: the many-cotangent mode of the search-free adjoint with PSD blocks and exponential / power triples
//   (k_backward_ns<..., TRI, MANY, PSD> without FWD), every row of CE_NS_VARIANTS (an object of its own beside ce_tu_ns_vjp_psd_many.hip: csrc/Makefile)
#include "ce_tu_prologue.h"
#include "ce_variants.h"
namespace {
#include "ce_backward_ns.h"
}  // namespace

int ce_launch_ns(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsVjpManyPsdTri &w) {
    switch (variant) {
#define X(V, NTILE, NTHR) case V: hipLaunchKernelGGL((k_backward_ns<NTILE, NTHR, false, false, false, true, true, true>), dim3(B), dim3(NTHR), lds, st, a.T, a.Abm, a.x, a.y, a.s, a.dx, a.dy, a.dA, a.dq, a.sdqk, a.sdqb, a.adj, a.fix, w); return 0;
        CE_NS_VARIANTS(X)
#undef X
    default: return -1;
    }
}
hipError_t ce_setattr_ns_vjp_psd_tri_many(int bytes) {
#define X(V, NTILE, NTHR) { const hipError_t e_ = ce_set_max_lds(&k_backward_ns<NTILE, NTHR, false, false, false, true, true, true>, bytes); if (e_ != hipSuccess) return e_; }
    CE_NS_VARIANTS(X)
#undef X
    return hipSuccess;
}
