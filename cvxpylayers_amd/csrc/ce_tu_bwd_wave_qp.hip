// translation unit: the one-instance-per-wave adjoint of small quadratic programs (k_bwd_wave_qp)
#include "ce_tu_prologue.h"
#include "ce_variants_bwd_wave_qp.h"
namespace {
#include "ce_backward_wave_qp.h"
}  // namespace

// one 64-thread workgroup (one wave) per instance, in index order; a.P / a.nnz_p: the instances' P rows, a.prow / a.pcol / a.p_tri: (row, column) of every entry of
// the P structure and whether it stores one triangle, a.dP: the instances' dP rows
int ce_launch_bwd_wave_qp(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a) {
    switch (variant) {
#define X(V, NX, MY, WPS) case V: hipLaunchKernelGGL((k_bwd_wave_qp<NX, MY, WPS>), dim3(B), dim3(64), lds, st, a.T, a.Abm, a.P, a.nnz_p, a.prow, a.pcol, a.p_tri, a.x, a.y, a.s, a.dx, a.dy, a.dA, a.dq, a.sdqk, a.sdqb, a.dP, a.adj); return 0;
        CE_BWD_WAVE_QP_VARIANTS(X)
#undef X
    default: return -1;
    }
}
// resident workgroups (= instances) per CU of row `variant` with `lds` bytes of dynamic LDS
hipError_t ce_occupancy_bwd_wave_qp(int variant, size_t lds, int *blocks) {
    *blocks = 0;
    switch (variant) {
#define X(V, NX, MY, WPS) case V: return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, reinterpret_cast<const void *>(&k_bwd_wave_qp<NX, MY, WPS>), 64, lds);
        CE_BWD_WAVE_QP_VARIANTS(X)
#undef X
    default: return hipErrorInvalidValue;
    }
}
