// translation unit: the one-instance-per-wave forward kernel of small templates (k_fwd_wave)
#include "ce_tu_prologue.h"
#include "ce_variants_wave.h"
namespace {
#include "ce_forward_wave.h"
}  // namespace

// one 64-thread workgroup (one wave) per instance, in index order
int ce_launch_fwd_wave(int variant, int B, size_t lds, hipStream_t st, const CeFwdArgs &a) {
    switch (variant) {
#define X(V, NX, MY, WPS) case V: hipLaunchKernelGGL((k_fwd_wave<NX, MY, WPS>), dim3(B), dim3(64), lds, st, a.T, a.S, a.Abm, a.q, a.sqk, a.sqb, a.x, a.y, a.s, a.iters, a.status, a.resid); return 0;
        CE_WAVE_VARIANTS(X)
#undef X
    default: return -1;
    }
}
// resident workgroups (= instances) per CU of row `variant` with `lds` bytes of dynamic LDS
hipError_t ce_occupancy_fwd_wave(int variant, size_t lds, int *blocks) {
    *blocks = 0;
    switch (variant) {
#define X(V, NX, MY, WPS) case V: return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks, reinterpret_cast<const void *>(&k_fwd_wave<NX, MY, WPS>), 64, lds);
        CE_WAVE_VARIANTS(X)
#undef X
    default: return hipErrorInvalidValue;
    }
}
