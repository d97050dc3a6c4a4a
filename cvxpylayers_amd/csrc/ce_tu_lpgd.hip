// translation unit: the LPGD backward's streaming kernels (k_lpgd_perturb, k_lpgd_grad_rows, k_lpgd_grad_tile)
//   (one object file: csrc/Makefile)
#include "ce_tu_prologue.h"
namespace {
#include "ce_lpgd.h"
}  // namespace

size_t ce_lpgd_grad_rows_lds(int n, int m) { return sizeof(double) * (size_t)VAL_IPB * (3 * (size_t)n + 2 * (size_t)m); }
size_t ce_lpgd_grad_tile_lds(int n, int m) { return sizeof(double) * (size_t)VAL_TLD * 2 * ((size_t)n + m); }

void ce_launch_lpgd_perturb(hipStream_t st, const CeLpgdPerturbArgs &a) {
    hipLaunchKernelGGL(k_lpgd_perturb, dim3((a.B + VAL_IPB - 1) / VAL_IPB), dim3(VAL_NT), 0, st, a);
}
void ce_launch_lpgd_grad_rows(size_t lds, hipStream_t st, const CeLpgdGradArgs &a) {
    hipLaunchKernelGGL(k_lpgd_grad_rows, dim3((a.B + VAL_IPB - 1) / VAL_IPB), dim3(VAL_NT), lds, st, a);
}
void ce_launch_lpgd_grad_tile(bool staged, int chunks, int kchunk, int wdq, size_t lds, hipStream_t st, const CeLpgdGradArgs &a) {
    const dim3 grid((a.B + VAL_TI - 1) / VAL_TI, chunks);
    if (staged) hipLaunchKernelGGL(k_lpgd_grad_tile<true>, grid, dim3(VAL_NT), lds, st, a, kchunk, wdq);
    else hipLaunchKernelGGL(k_lpgd_grad_tile<false>, grid, dim3(VAL_NT), 0, st, a, kchunk, wdq);
}
hipError_t ce_setattr_lpgd(int bytes) {
    hipError_t e = ce_set_max_lds(&k_lpgd_grad_rows, bytes); if (e != hipSuccess) return e;
    return ce_set_max_lds(&k_lpgd_grad_tile<true>, bytes);
}
