// ce_cone_proj_triple.h -- one exponential / 3-d power triple of the stand-alone cone projection: the projection from a cold root and, when wanted, its 3 x 3
// Jacobian.  Plain C++ apart from the qualifiers, like ce_expcone.h whose routines it calls (tests/test_cone_proj_host.py runs it on the host).
#pragma once
#include "ce_expcone.h"

// out = Pi(v), J (row-major 3 x 3, or null) = D Pi(v), for the cone of a set's entry:
//   is_exp: the exponential cone; else the power cone of entry a (a > 0: K_a, a < 0: the dual cone K_|a|^*, the convention of ce_template.p);
//   dual  : project onto the DUAL of that cone instead.
// A dual-cone projection goes through Moreau exactly as k_ca_triple_jac does: Pi_K*(v) = v + Pi_K(-v), D Pi_K*(v) = I - D Pi_K(-v).
// A non-finite input gives NaN everywhere and runs no iteration.  Every loop below has a static trip count; the Newton iterations of exp_project /
// pow_project are capped at 120 (ce_expcone.h).
__device__ __forceinline__ void cone_triple_project(const double *v, bool is_exp, double a, int dual, double *out, double *J) {
    const double v0 = v[0], v1 = v[1], v2 = v[2];
    if (!(fabs(v0) < INFINITY && fabs(v1) < INFINITY && fabs(v2) < INFINITY)) {
        out[0] = out[1] = out[2] = NAN;
        if (J) for (int i = 0; i < 9; i++) J[i] = NAN;
        return;
    }
    const bool onto_dual = is_exp ? (dual != 0) : ((a < 0) != (dual != 0));
    const double al = fabs(a), sg = onto_dual ? -1.0 : 1.0;
    const double w[3] = {sg * v0, sg * v1, sg * v2};
    double p0 = w[0], p1 = w[1], p2 = w[2];
    if (is_exp) { ExpInfo inf; exp_project(p0, p1, p2, 0.0, inf); }
    else { double r = -1.0; pow_project(p0, p1, p2, al, r); }
    if (onto_dual) { out[0] = v0 + p0; out[1] = v1 + p1; out[2] = v2 + p2; }
    else { out[0] = p0; out[1] = p1; out[2] = p2; }
    if (!J) return;
    if (is_exp) exp_dproject(w, J); else pow_dproject(w, al, J);
    if (onto_dual) for (int i = 0; i < 9; i++) J[i] = ((i % 4 == 0) ? 1.0 : 0.0) - J[i];
}
