// ce_lds_common.h -- sizes and LDS footprints that more than one kernel family and the launch plan (ce_plan.h) share.  Plain C++ apart from the
// __host__ __device__ qualifiers (no HIP include): the kernels carve with these numbers, the plan sums them.  Included inside an anonymous namespace.
#pragma once

constexpr int NT = 256;            // threads per workgroup
constexpr int NW = NT / 64;        // waves per workgroup
constexpr int SOC_SMALL = 32;   // cones up to this size: every row thread recomputes its cone's norm (no extra barrier)

// LDS doubles of the blocked Gauss-Jordan panels (G in global memory): column panel NP16 x 17, pivot block 16 x 17
__host__ __device__ inline size_t generic_gj_panel_doubles(int n) { const int np16 = 16 * ((n + 15) / 16); return (size_t)np16 * 17 + 16 * 17 + 2; }

// LDS doubles of the blocked pivoted elimination (generic backward kernel, K in global memory): column panel nkcap x 17, two 16 x 17 blocks, pivots
__host__ __device__ inline size_t generic_lu_panel_doubles(int nkcap) { return (size_t)nkcap * 17 + 2 * 16 * 17 + (size_t)nkcap + 2; }

// LDS doubles the forward kernels add for PSD / exponential / power cones: the Jacobi scratch of psd_project (S, V, (c, s, p, q) per pair) and one root per triple
__host__ __device__ inline size_t fwd_cone_scratch_doubles(int ns, int maxs, int ntri) { return (ns > 0 ? 2 * (size_t)maxs * maxs + 2 * (size_t)maxs + 8 : 0) + (size_t)ntri; }
// ... and the elimination adjoints (k_backward, k_backward_rt<PSD>): eigenvectors and eigenvalues per PSD cone, the DPi eigenvalue of every row, one (X, W) pair
// per wave plus the Jacobi scratch, the 3 x 3 eigenvector matrix of every triple
__host__ __device__ inline size_t bwd_cone_scratch_doubles(int ns, int maxs, int m, int ntri, int nwaves) {
    if (ns == 0 && ntri == 0) return 0;
    return (size_t)ns * maxs * maxs + (size_t)ns * maxs + m + 2 * (size_t)nwaves * maxs * maxs + 2 * maxs + 8 + 9 * (size_t)ntri;
}
__host__ __device__ constexpr int imax(int a, int b) { return a > b ? a : b; }
