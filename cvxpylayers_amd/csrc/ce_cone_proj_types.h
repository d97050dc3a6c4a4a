// ce_cone_proj_types.h -- what the host entry points of the stand-alone cone projection (ce_cones_create, ce_cone_project, ce_cone_dproject) hand the kernels of
// ce_cone_proj.h.  A projection needs no template matrix: the handle owns the cone layout alone.
#pragma once
#include "ce_lds_cone_proj.h"

// the cone layout on the device (uploaded once by ce_cones_create); rows are relative to an instance's first row
struct ConeProjDev {
    int z, l, nq, ns, nep, np;
    int nq_small, nq_large;       // second-order cones of dimension <= / > CONE_PROJ_SOC_SMALL
    int e_row0;                   // first row of the triples
    long long state_len, tri_state0;
    const int *qoff;              // [nq + 1] first row of every second-order cone
    const int *soc_small, *soc_large;     // [nq_small], [nq_large] cone indices of each lane shape
    const int *sord, *soff;       // [ns] PSD orders, [ns + 1] first rows
    const long long *sstate;      // [ns] state offset of every PSD block
    const double *pw;             // [np] power-cone entries
};
// one call: out = Pi(v) (state: written when non-null) or out = D Pi(v) dir (state: read).  Row pitches in elements.
struct ConeProjArgs {
    ConeProjDev D;
    int B, dual;
    const double *v; long ldv;
    const double *dir; long lddir;
    double *out; long ldout;
    double *state;
};
