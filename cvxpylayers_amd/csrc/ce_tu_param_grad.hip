// translation unit: parameter gradients straight from the adjoint's factors (k_param_grad), the four tile sizes
//   (one object file: csrc/Makefile; not a tiled family: no row in ce_variants.h)
#include "ce_tu_prologue.h"
namespace {
#include "ce_param_grad.h"
constexpr size_t PG_LDS_MAX = 160 * 1024 - 512, PG_LDS_TWO = 80 * 1024;          // the kernel's dynamic-LDS limit; two workgroups per CU
}  // namespace

// tile: the largest of 16, 8, 4, 2 pairs that leaves two workgroups per CU, else 2.  Slabs of rows so that tiles x slabs is about four workgroups per CU (as
// k_expand_dA plans), no slab shorter than one pass of the workgroup's lanes.
int ce_launch_param_grad(hipStream_t st, const CeParamGradArgs &a0) {
    CeParamGradArgs a = a0;
    const long npairs = (long)a.K * a.B;
    const int maxslabs = (a.rows + PG_NT - 1) / PG_NT;
    for (int tp = PG_TP_MAX; tp >= 2; tp >>= 1) {
        const long tiles = (npairs + tp - 1) / tp;
        const int slabs = (int)std::max<long>((a.rows + 2047) / 2048, std::min<long>(maxslabs, (1024 + tiles - 1) / tiles));      // (at most 2048 rows: the list of long rows is the slab's size)
        a.slab = (a.rows + slabs - 1) / slabs;
        const int ny = (a.rows + a.slab - 1) / a.slab;
        const size_t lds = param_grad_lds_bytes(a.n, a.m, a.slab, tp);
        if (lds > (tp > 2 ? PG_LDS_TWO : PG_LDS_MAX)) continue;
        const dim3 grid((unsigned)tiles, (unsigned)ny);
        switch (tp) {
        case 16: hipLaunchKernelGGL(k_param_grad<16>, grid, dim3(PG_NT), lds, st, a); break;
        case 8: hipLaunchKernelGGL(k_param_grad<8>, grid, dim3(PG_NT), lds, st, a); break;
        case 4: hipLaunchKernelGGL(k_param_grad<4>, grid, dim3(PG_NT), lds, st, a); break;
        default: hipLaunchKernelGGL(k_param_grad<2>, grid, dim3(PG_NT), lds, st, a); break;
        }
        return 0;
    }
    return -1;
}
hipError_t ce_setattr_param_grad(int bytes) {
    bytes = std::min(bytes, (int)PG_LDS_MAX);
    hipError_t e = ce_set_max_lds(&k_param_grad<16>, bytes); if (e != hipSuccess) return e;
    e = ce_set_max_lds(&k_param_grad<8>, bytes); if (e != hipSuccess) return e;
    e = ce_set_max_lds(&k_param_grad<4>, bytes); if (e != hipSuccess) return e;
    return ce_set_max_lds(&k_param_grad<2>, bytes);
}
