// translation unit: first-generation register-tiled forward kernel (k_forward_rt) and the size-generic forward kernel (k_forward)
#include "ce_tu_prologue.h"
#include "ce_variants.h"
namespace {
#include "ce_forward_rt.h"
#include "ce_forward_generic.h"
}  // namespace

int ce_launch_fwd_rt(int variant, int B, size_t lds, hipStream_t st, const CeFwdArgs &a) {
    switch (variant) {
#define X(V, ...) case V: hipLaunchKernelGGL((k_forward_rt<__VA_ARGS__>), dim3(B), dim3(NT2), lds, st, a.T, a.S, a.Abm, a.q, a.sqk, a.sqb, a.x, a.y, a.s, a.iters, a.status, a.resid, a.aa_ws); return 0;
        CE_RT_VARIANTS(X)
#undef X
    default: return -1;
    }
}
int ce_launch_fwd_generic(int mode, int B, size_t lds, hipStream_t st, const CeFwdArgs &a) {
#define LAUNCH_F(AL, GL) hipLaunchKernelGGL((k_forward<AL, GL>), dim3(B), dim3(NT), lds, st, a.T, a.S, a.Abm, a.q, a.sqk, a.sqb, a.x, a.y, a.s, a.iters, a.status, a.resid, a.gA, a.gG, a.aa_ws)
    switch (mode) {
    case 0: LAUNCH_F(true, true); break;
    case 1: LAUNCH_F(true, false); break;
    case 2: LAUNCH_F(false, false); break;
    default: return -1;
    }
#undef LAUNCH_F
    return 0;
}
#define SETATTR(kern) do { const hipError_t e_ = ce_set_max_lds(&kern, bytes); if (e_ != hipSuccess) return e_; } while (0)
hipError_t ce_setattr_fwd_rt(int bytes) {
#define X(V, ...) SETATTR((k_forward_rt<__VA_ARGS__>));
    CE_RT_VARIANTS(X)
#undef X
    return hipSuccess;
}
hipError_t ce_setattr_fwd_generic(int bytes) {
    SETATTR((k_forward<true, true>)); SETATTR((k_forward<true, false>)); SETATTR((k_forward<false, false>));
    return hipSuccess;
}
