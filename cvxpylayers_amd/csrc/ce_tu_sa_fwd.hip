// translation unit: shared-A forward kernel (k_sa_fwd)
#include "ce_tu_prologue.h"
#include "ce_variants.h"
namespace {
#include "ce_shared_a_fwd.h"
}  // namespace

int ce_launch_sa_fwd(int variant, int B, size_t lds, hipStream_t st, const CeSaFwdArgs &a) {
    switch (variant) {
#define X(V, RP, NTH, CIDX, HTRI) \
    case V: hipLaunchKernelGGL((k_sa_fwd<RP, NTH, CIDX != 0, HTRI != 0>), dim3(B), dim3(NTH), lds, st, a.T, a.F, a.S, a.b_hat, a.c_hat, a.sigma, a.nrm_b0, a.nrm_c0, \
                               a.warm_x, a.warm_y, a.warm_s, a.x, a.y, a.s, a.iters, a.status, a.resid); return 0;
        CE_SA_FWD_VARIANTS(X)
#undef X
    default: return -1;
    }
}
#define SETATTR(kern) do { const hipError_t e_ = ce_set_max_lds(&kern, bytes); if (e_ != hipSuccess) return e_; } while (0)
hipError_t ce_setattr_sa_fwd(int bytes) {
#define X(V, RP, NTH, CIDX, HTRI) SETATTR((k_sa_fwd<RP, NTH, CIDX != 0, HTRI != 0>));
    CE_SA_FWD_VARIANTS(X)
#undef X
    return hipSuccess;
}
