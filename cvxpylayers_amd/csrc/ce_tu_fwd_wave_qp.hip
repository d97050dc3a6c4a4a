// translation unit: the one-instance-per-wave forward kernel of small quadratic programs (k_fwd_wave_qp)
#include "ce_tu_prologue.h"
#include "ce_variants_fwd_wave_qp.h"
namespace {
#include "ce_forward_wave_qp.h"
}  // namespace

// one 64-thread workgroup (one wave) per instance, in index order; a.P / a.nnz_p: the instances' P rows, prow / pcol / p_tri: (row, column) of every entry of the
// P structure and whether it stores one triangle
int ce_launch_fwd_wave_qp(int variant, int B, size_t lds, hipStream_t st, const CeFwdArgs &a, const int *prow, const int *pcol, int p_tri) {
    switch (variant) {
#define X(V, NX, MY, WPS) case V: hipLaunchKernelGGL((k_fwd_wave_qp<NX, MY, WPS>), dim3(B), dim3(64), lds, st, a.T, a.S, a.Abm, a.q, a.sqk, a.sqb, a.P, a.nnz_p, prow, pcol, p_tri, a.x, a.y, a.s, a.iters, a.status, a.resid); return 0;
        CE_FWD_WAVE_QP_VARIANTS(X)
#undef X
    default: return -1;
    }
}
// resident workgroups (= instances) per CU of row `variant` with `lds` bytes of dynamic LDS
hipError_t ce_occupancy_fwd_wave_qp(int variant, size_t lds, int *blocks) {
    *blocks = 0;
    switch (variant) {
#define X(V, NX, MY, WPS) case V: return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, reinterpret_cast<const void *>(&k_fwd_wave_qp<NX, MY, WPS>), 64, lds);
        CE_FWD_WAVE_QP_VARIANTS(X)
#undef X
    default: return hipErrorInvalidValue;
    }
}
