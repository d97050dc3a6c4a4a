// ce_lds_psd_mfma.h -- pitches and scratch sizes of the MFMA PSD projections (ce_psd_mfma.h), as the shared-A footprints and the host's k_ca_psd_mfma launch use them.
// Plain C++ apart from the qualifiers.
#pragma once

__host__ __device__ inline int psd_refine_pitch(int k) { return k | 1; }                 // odd pitch: the strided operand reads spread over the banks
// LDS doubles of the scratch shared by all blocks of an instance (S, T / E, D, R + rotation parameters + eigenvalues + lam); every block keeps k P more (V)
__host__ __device__ inline int psd_refine_scratch_doubles(int kmax) { return 4 * kmax * psd_refine_pitch(kmax) + 4 * kmax + 16; }

// LDS doubles needed: 3 * KP * (KP + 1) + 2 * k + 8  (+ the reduction scratch of block_reduce_n)
__host__ __device__ inline int psd_mfma_kp(int k) { return 16 * ((k + 15) / 16); }
