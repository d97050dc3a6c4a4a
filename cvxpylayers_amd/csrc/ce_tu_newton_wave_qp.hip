// translation unit: the one-instance-per-wave forward derivative and Newton refinement step of small quadratic programs (k_newton_wave_qp, both modes of every row)
#include "ce_tu_prologue.h"
#include "ce_variants_newton_wave_qp.h"
namespace {
#include "ce_newton_wave_qp.h"
}  // namespace

// one 64-thread workgroup (one wave) per instance, in index order: the forward derivative; q: the instances' P rows, their tangent and the P structure
int ce_launch_newton_wave_qp(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsJvp &w, const NwQp &q) {
    switch (variant) {
#define X(V, NX, MY, WPS, WPSR) case V: hipLaunchKernelGGL((k_newton_wave_qp<NX, MY, WPS, false>), dim3(B), dim3(64), lds, st, a.T, a.Abm, q, a.x, a.y, a.s, a.adj, w); return 0;
        CE_NEWTON_WAVE_QP_VARIANTS(X)
#undef X
    default: return -1;
    }
}
// the same grid: one safeguarded Newton step (x, y, s are w's, in / out)
int ce_launch_newton_wave_qp(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsRefine &w, const NwQp &q) {
    switch (variant) {
#define X(V, NX, MY, WPS, WPSR) case V: hipLaunchKernelGGL((k_newton_wave_qp<NX, MY, WPSR, true>), dim3(B), dim3(64), lds, st, a.T, a.Abm, q, nullptr, nullptr, nullptr, nullptr, w); return 0;
        CE_NEWTON_WAVE_QP_VARIANTS(X)
#undef X
    default: return -1;
    }
}
// resident workgroups (= instances) per CU of row `variant` and mode with `lds` bytes of dynamic LDS
hipError_t ce_occupancy_newton_wave_qp(int variant, int refine, size_t lds, int *blocks) {
    *blocks = 0;
    switch (variant) {
#define X(V, NX, MY, WPS, WPSR) case V: return refine ? hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, reinterpret_cast<const void *>(&k_newton_wave_qp<NX, MY, WPSR, true>), 64, lds) \
                                                : hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, reinterpret_cast<const void *>(&k_newton_wave_qp<NX, MY, WPS, false>), 64, lds);
        CE_NEWTON_WAVE_QP_VARIANTS(X)
#undef X
    default: return hipErrorInvalidValue;
    }
}
