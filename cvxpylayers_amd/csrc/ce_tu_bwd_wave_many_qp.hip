// translation unit: the many-cotangent adjoint of small quadratic programs, one wave per (instance, chunk of cotangents) (k_bwd_wave_many_qp)
#include "ce_tu_prologue.h"
#include "ce_variants_bwd_wave_many_qp.h"
namespace {
#include "ce_backward_wave_many_qp.h"
}  // namespace

// one 64-thread workgroup (one wave) per instance and chunk of KC cotangents: blockIdx.x the instance, blockIdx.y the chunk; w carries the strides, the record
// fields, the instances' P rows, the P structure's (row, column) arrays and the dP rows
int ce_launch_bwd_wave_many_qp(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const BwdWaveManyQp &w) {
    if (w.K < 1) return -1;
    switch (variant) {
#define X(V, NX, MY, KC, WPS) case V: hipLaunchKernelGGL((k_bwd_wave_many_qp<NX, MY, KC, WPS>), dim3(B, (w.K + KC - 1) / KC), dim3(64), lds, st, a.T, a.Abm, a.x, a.y, a.s, a.dx, a.dy, a.dA, a.dq, a.sdqk, a.sdqb, a.adj, w); return 0;
        CE_BWD_WAVE_MANY_QP_VARIANTS(X)
#undef X
    default: return -1;
    }
}
// resident workgroups (= instance-chunks) per CU of row `variant` with `lds` bytes of dynamic LDS
hipError_t ce_occupancy_bwd_wave_many_qp(int variant, size_t lds, int *blocks) {
    *blocks = 0;
    switch (variant) {
#define X(V, NX, MY, KC, WPS) case V: return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, reinterpret_cast<const void *>(&k_bwd_wave_many_qp<NX, MY, KC, WPS>), 64, lds);
        CE_BWD_WAVE_MANY_QP_VARIANTS(X)
#undef X
    default: return hipErrorInvalidValue;
    }
}
