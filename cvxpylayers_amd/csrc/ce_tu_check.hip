// translation unit: the forward kernels' termination test at a given point (k_check_solved, k_check_count)
//   (one object file: csrc/Makefile)
#include "ce_tu_prologue.h"
namespace {
#include "ce_check.h"
}  // namespace

size_t ce_check_lds(int n, int m, int nnz_staged) { return sizeof(double) * (3 * ((size_t)n + m) + CHK_NT + CHK_NW * CHK_NQ + (size_t)nnz_staged); }

void ce_launch_check_solved(bool staged, size_t lds, hipStream_t st, const CeCheckArgs &a, int *n_unsolved) {
    if (staged) hipLaunchKernelGGL(k_check_solved<true>, dim3(a.B), dim3(CHK_NT), lds, st, a);
    else hipLaunchKernelGGL(k_check_solved<false>, dim3(a.B), dim3(CHK_NT), lds, st, a);
    hipLaunchKernelGGL(k_check_count, dim3(1), dim3(CHK_NT), 0, st, a.B, (const unsigned char *)a.solved, n_unsolved);
}
hipError_t ce_setattr_check(int bytes) {
    hipError_t e = ce_set_max_lds(&k_check_solved<true>, bytes); if (e != hipSuccess) return e;
    return ce_set_max_lds(&k_check_solved<false>, bytes);
}
