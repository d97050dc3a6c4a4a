// translation unit: shared-A / per-instance LSQR adjoint and forward derivative (k_sa_lsqr), and the refill of the split's values (k_sa_fill_split)
#include "ce_tu_prologue.h"
#include "ce_variants.h"
namespace {
#include "ce_shared_a.h"
}  // namespace

int ce_launch_sa_lsqr(int variant, int grid, size_t lds, hipStream_t st, const CeSaLsqrArgs &a) {
    switch (variant) {
#define X(V, RP, HPSD, HTRI, LSMR, FWD) \
    case V: hipLaunchKernelGGL((k_sa_lsqr<RP, HPSD != 0, HTRI != 0, LSMR != 0, FWD != 0>), dim3(grid), dim3(NT), lds, st, a.T, a.S, a.F, a.A_vals0, a.sA_b, a.per_inst, a.q, a.sqk, a.sqb, \
                               a.x, a.y, a.s, a.dx, a.dy, a.dA, a.dq, a.sdqk, a.sdqb, a.adj, a.iters, a.atol, a.btol, a.conlim, a.iter_lim, a.sel, a.status_or, a.a_lds, a.sel_reset, a.W, a.M); return 0;
        CE_SA_LSQR_VARIANTS(X)
#undef X
    default: return -1;
    }
}
void ce_launch_sa_fill_split(hipStream_t st, int nnzA, int RP, const int *rowidx, const int *colidx, const int *rowslot, const double *vals, double *AdT, double *srow_val,
                             const int *sing_i, double *sing_v) {
    hipLaunchKernelGGL(k_sa_fill_split, dim3((nnzA + 255) / 256), dim3(256), 0, st, nnzA, RP, rowidx, colidx, rowslot, vals, AdT, srow_val, sing_i, sing_v);
}
#define SETATTR(kern) do { const hipError_t e_ = ce_set_max_lds(&kern, bytes); if (e_ != hipSuccess) return e_; } while (0)
hipError_t ce_setattr_sa_lsqr(int bytes) {
#define X(V, RP, HPSD, HTRI, LSMR, FWD) SETATTR((k_sa_lsqr<RP, HPSD != 0, HTRI != 0, LSMR != 0, FWD != 0>));
    CE_SA_LSQR_VARIANTS(X)
#undef X
    return hipSuccess;
}
