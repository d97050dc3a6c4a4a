// translation unit: register-tiled structured adjoint (k_backward_rt)
//   -DCE_BRT_PSD=0 plain cones, 1 PSD / exponential / power cones (one object file each: csrc/Makefile)
#include "ce_tu_prologue.h"
#include "ce_variants.h"
namespace {
#include "ce_backward_rt.h"
}  // namespace

#ifndef CE_BRT_PSD
#error "compile with -DCE_BRT_PSD=0|1"
#endif
#define BRT_ARGS a.T, a.Abm, a.x, a.y, a.s, a.dx, a.dy, a.dA, a.dq, a.sdqk, a.sdqb, a.adj, a.P, a.nnz_p, a.pmap, a.prow, a.pcol, a.p_tri, a.dP, a.retry, a.nk_max, a.fix, a.nonfinal
#define SETATTR(kern) do { const hipError_t e_ = ce_set_max_lds(&kern, bytes); if (e_ != hipSuccess) return e_; } while (0)

namespace {
// a row of CE_BRT_VARIANTS is instantiated for this object's kind (every row for plain cones, the rows marked PSD for the other); `if constexpr` on the
// template parameter discards the other rows' kernels at compile time
template <bool PSD>
int launch_brt(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a) {
    switch (variant) {
#define X(V, TI, TJ, TH, BGR, PSD_ROW) \
    case V: if constexpr (!PSD || PSD_ROW) { hipLaunchKernelGGL((k_backward_rt<TI, TJ, TH, PSD, BGR>), dim3(B), dim3(BGR * BGC), lds, st, BRT_ARGS); return 0; } return -1;
        CE_BRT_VARIANTS(X)
#undef X
    default: return -1;
    }
}
template <bool PSD>
hipError_t setattr_brt(int bytes) {
#define X(V, TI, TJ, TH, BGR, PSD_ROW) if constexpr (!PSD || PSD_ROW) SETATTR((k_backward_rt<TI, TJ, TH, PSD, BGR>));
    CE_BRT_VARIANTS(X)
#undef X
    return hipSuccess;
}
}  // namespace

#if CE_BRT_PSD == 0
int ce_launch_bwd_rt_plain(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a) { return launch_brt<CE_BRT_PSD != 0>(variant, B, lds, st, a); }
hipError_t ce_setattr_bwd_rt_plain(int bytes) { return setattr_brt<CE_BRT_PSD != 0>(bytes); }
#else
int ce_launch_bwd_rt_psd(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a) { return launch_brt<CE_BRT_PSD != 0>(variant, B, lds, st, a); }
hipError_t ce_setattr_bwd_rt_psd(int bytes) { return setattr_brt<CE_BRT_PSD != 0>(bytes); }
#endif
