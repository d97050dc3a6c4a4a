// translation unit: second-generation forward kernel (k_fwd2), all instantiations of one `kind`
//   -DCE_F2_KIND=0 plain cones, 1 PSD / exponential / power cones, 2 quadratic objective   (one object file per kind: csrc/Makefile)
#include "ce_tu_prologue.h"
#include "ce_variants.h"
namespace {
#include "ce_forward_v2.h"
}  // namespace

#ifndef CE_F2_KIND
#error "compile with -DCE_F2_KIND=0|1|2"
#endif

// the kernel of a row of CE_F2_VARIANTS for this object's kind, and whether the row is instantiated for it
#if CE_F2_KIND == 0
#define F2_KERNEL(CHT, T1, CHA, T2, CHG, TG, NTH, WL) k_fwd2<CHT, T1, CHA, T2, CHG, TG, false, NTH, false, WL>
#define F2_HAS(WL_ROW, QP_ROW) (!WL || WL_ROW)
#elif CE_F2_KIND == 1
#define F2_KERNEL(CHT, T1, CHA, T2, CHG, TG, NTH, WL) k_fwd2<CHT, T1, CHA, T2, CHG, TG, true, NTH, false, false>
#define F2_HAS(WL_ROW, QP_ROW) true
#else
#define F2_KERNEL(CHT, T1, CHA, T2, CHG, TG, NTH, WL) k_fwd2<CHT, T1, CHA, T2, CHG, TG, false, NTH, true, false>
#define F2_HAS(WL_ROW, QP_ROW) (QP_ROW != 0)
#endif

#define F2_ARGS a.T, a.S, a.Abm, a.q, a.sqk, a.sqb, a.idx_at, a.idx_ar, a.idx_b, a.x, a.y, a.s, a.iters, a.status, a.resid, a.P, a.nnz_p, a.idx_p, a.row_perm, a.order, a.iters2
namespace {
template <bool WL>      // WL: rows packed so that every cone is wave-local (plain kind only)
int launch_f2(int variant, int B, size_t lds, hipStream_t st, const CeFwdArgs &a) {
    switch (variant) {
#define X(V, CHT, T1, CHA, T2, CHG, TG, NTH, WL_ROW, QP_ROW) \
    case V: if constexpr (F2_HAS(WL_ROW, QP_ROW)) { hipLaunchKernelGGL((F2_KERNEL(CHT, T1, CHA, T2, CHG, TG, NTH, WL)), dim3(B), dim3(NTH), lds, st, F2_ARGS); return 0; } return -1;
        CE_F2_VARIANTS(X)
#undef X
    default: return -1;
    }
}
template <bool WL>
hipError_t setattr_f2(int bytes) {
#define X(V, CHT, T1, CHA, T2, CHG, TG, NTH, WL_ROW, QP_ROW) \
    if constexpr (F2_HAS(WL_ROW, QP_ROW)) { const hipError_t e_ = ce_set_max_lds(&F2_KERNEL(CHT, T1, CHA, T2, CHG, TG, NTH, WL), bytes); if (e_ != hipSuccess) return e_; }
    CE_F2_VARIANTS(X)
#undef X
    return hipSuccess;
}
}  // namespace

#if CE_F2_KIND == 0
int ce_launch_fwd2_plain(int variant, int B, size_t lds, hipStream_t st, const CeFwdArgs &a) { return a.row_perm ? launch_f2<true>(variant, B, lds, st, a) : launch_f2<false>(variant, B, lds, st, a); }
hipError_t ce_setattr_fwd2_plain(int bytes) { const hipError_t e = setattr_f2<false>(bytes); return e != hipSuccess ? e : setattr_f2<true>(bytes); }
#elif CE_F2_KIND == 1
int ce_launch_fwd2_psd(int variant, int B, size_t lds, hipStream_t st, const CeFwdArgs &a) { return launch_f2<false>(variant, B, lds, st, a); }
hipError_t ce_setattr_fwd2_psd(int bytes) { return setattr_f2<false>(bytes); }
#else
int ce_launch_fwd2_qp(int variant, int B, size_t lds, hipStream_t st, const CeFwdArgs &a) { return launch_f2<false>(variant, B, lds, st, a); }
hipError_t ce_setattr_fwd2_qp(int bytes) { return setattr_f2<false>(bytes); }
#endif
