// translation unit: the optimal value of an instance and its envelope-theorem derivatives (k_value, k_value_vjp_rows, k_value_vjp_tile)
//   (one object file: csrc/Makefile)
#include "ce_tu_prologue.h"
namespace {
#include "ce_value.h"
}  // namespace

size_t ce_value_lds(int n, int m) { return sizeof(double) * ((size_t)n + m + VAL_NT); }
size_t ce_value_vjp_rows_lds(int n, int m) { return sizeof(double) * ((size_t)VAL_IPB * ((size_t)n + m) + VAL_IPB); }
size_t ce_value_vjp_tile_lds(int n, int m) { return sizeof(double) * ((size_t)VAL_TLD * ((size_t)n + m) + VAL_TI); }

void ce_launch_value(bool jvp, size_t lds, hipStream_t st, const CeValueArgs &a) {
    if (jvp) hipLaunchKernelGGL(k_value<true>, dim3(a.B), dim3(VAL_NT), lds, st, a);
    else hipLaunchKernelGGL(k_value<false>, dim3(a.B), dim3(VAL_NT), lds, st, a);
}
void ce_launch_value_vjp_rows(size_t lds, hipStream_t st, const CeValueVjpArgs &a) {
    hipLaunchKernelGGL(k_value_vjp_rows, dim3((a.B + VAL_IPB - 1) / VAL_IPB), dim3(VAL_NT), lds, st, a);
}
void ce_launch_value_vjp_tile(bool staged, int chunks, int kchunk, int wdq, size_t lds, hipStream_t st, const CeValueVjpArgs &a) {
    const dim3 grid((a.B + VAL_TI - 1) / VAL_TI, chunks);
    if (staged) hipLaunchKernelGGL(k_value_vjp_tile<true>, grid, dim3(VAL_NT), lds, st, a, kchunk, wdq);
    else hipLaunchKernelGGL(k_value_vjp_tile<false>, grid, dim3(VAL_NT), 0, st, a, kchunk, wdq);
}
hipError_t ce_setattr_value(int bytes) {
    hipError_t e = ce_set_max_lds(&k_value<false>, bytes); if (e != hipSuccess) return e;
    e = ce_set_max_lds(&k_value<true>, bytes); if (e != hipSuccess) return e;
    e = ce_set_max_lds(&k_value_vjp_rows, bytes); if (e != hipSuccess) return e;
    return ce_set_max_lds(&k_value_vjp_tile<true>, bytes);
}
