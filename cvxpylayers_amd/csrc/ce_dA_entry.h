// ce_dA_entry.h -- one entry of the adjoint's dA row in the boundary convention, stated once for the two kernels that evaluate it: k_backward_ns's batch-major
// output loop (ce_backward_ns.h) and the batch-minor expansion from the factor vectors (k_expand_dA, ce_layout_kernels.h).  Both must produce the same bits.
#pragma once

// dA_eval[k] of the structural entry (i, j), j < n:  -(x_j r_y,i - y_i r_x,j).  Written out as one multiply and one fma so that no compiler decides the
// contraction per kernel: t = y r, then fma(x, v, -t), then the sign -- the form the output loop compiled to before this header existed (fp-contract=fast:
// v_mul_f64, v_fma_f64 with a negated addend, the sign folded into the select), so the values are unchanged.  The b column (j == n) is -v: the caller selects.
__device__ __forceinline__ double ce_dA_entry(double x, double v, double y, double r) { return -fma(x, v, -(y * r)); }

// dA_eval[k] of a structural entry (i, n) of the b column:  db_i = y_i r_tau - r_y,i.  One fma, the form the LSQR re-solve's epilogue writes (ce_shared_a.h); the
// elimination pins r_tau to 0, where this is -r_y,i: the -v its output loop and k_expand_dA store.  Stated here for the kernel that evaluates both kinds of entry
// from the factor records (k_param_grad, ce_param_grad.h).
__device__ __forceinline__ double ce_db_entry(double y, double rt, double v) { return fma(y, rt, -v); }

// dP[k] of the structural entry (i, j) of a quadratic objective's P (one share; the caller doubles a one-triangle entry with i != j):  -1/2 (r_x,i x_j + r_x,j x_i).
// One multiply, one fma and the scaling, in the order the many-cotangent QP adjoint's epilogue compiled to before this function existed (fp-contract=fast:
// v_mul_f64 r_x,j x_i, v_fmac_f64 r_x,i x_j onto it, v_mul_f64 by -0.5; the doubling a v_add_f64 of the result with itself behind a select), so ce_vjp_qp_many's dP
// keeps its bits.  Shared by that epilogue (ce_backward_ns.h) and k_param_grad (ce_param_grad.h), which evaluates the entries the P map touches from the records.
__device__ __forceinline__ double ce_dP_entry(double ri, double xj, double rj, double xi) { return -0.5 * fma(ri, xj, rj * xi); }
