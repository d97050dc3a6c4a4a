// translation unit: the many-tangent forward derivative of small templates, one wave per (instance, chunk of tangents) (k_jvp_wave_many)
#include "ce_tu_prologue.h"
#include "ce_variants_jvp_wave_many.h"
namespace {
#include "ce_jvp_wave_many.h"
}  // namespace

// one 64-thread workgroup (one wave) per instance and chunk of KC tangents: blockIdx.x the instance, blockIdx.y the chunk
int ce_launch_jvp_wave_many(int variant, int B, size_t lds, hipStream_t st, const CeBwdArgs &a, const NsJvpMany &w) {
    if (w.K < 1) return -1;
    switch (variant) {
#define X(V, NX, MY, KC, WPS) case V: hipLaunchKernelGGL((k_jvp_wave_many<NX, MY, KC, WPS>), dim3(B, (w.K + KC - 1) / KC), dim3(64), lds, st, a.T, a.Abm, a.x, a.y, a.s, a.adj, a.fix, w); return 0;
        CE_JVP_WAVE_MANY_VARIANTS(X)
#undef X
    default: return -1;
    }
}
// resident workgroups (= instance-chunks) per CU of row `variant` with `lds` bytes of dynamic LDS
hipError_t ce_occupancy_jvp_wave_many(int variant, size_t lds, int *blocks) {
    *blocks = 0;
    switch (variant) {
#define X(V, NX, MY, KC, WPS) case V: return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, reinterpret_cast<const void *>(&k_jvp_wave_many<NX, MY, KC, WPS>), 64, lds);
        CE_JVP_WAVE_MANY_VARIANTS(X)
#undef X
    default: return hipErrorInvalidValue;
    }
}
