// ce_lds_fwd2.h -- k_fwd2 (ce_forward_v2.h): the compile-time LDS layout of a variant (F2<>), the same numbers as data (F2Geom) and the fit test of the launch plan.
// Plain C++ apart from the qualifiers.
#pragma once
#include "ce_lds_common.h"

template <int CHT, int T1, int CHA, int T2, int CHG, int TG, int NWARP = 4>
struct F2 {
    static constexpr int MP = CHT * T1;                       // padded rows
    static constexpr int NPa = CHA * T2, NPg = CHG * TG;
    static constexpr int NP = NPa > NPg ? NPa : NPg;          // padded columns
    static constexpr int VP = MP + NP + 2;                    // one (y | x | tau) vector
    static constexpr int OY = 0, OX = MP, OT = MP + NP;
    static constexpr int O_W = 0, O_UT = VP, O_U = 2 * VP, O_ZB = 3 * VP, O_GV = 4 * VP, O_PHI = 5 * VP;
    static constexpr int O_BV = 6 * VP, O_DV = O_BV + MP, O_CV = O_DV + MP, O_EV = O_CV + NP, O_TV = O_EV + NP, O_PX = O_TV + NP,
                         O_S1 = O_PX + NP, O_S2 = O_S1 + NP, O_S3 = O_S2 + NP, O_S4 = O_S3 + NP,
                         O_RED = O_S4 + NP, O_WP = O_RED + NWARP * 8, O_SC = O_WP + NWARP, O_MT = O_SC + 16, O_G = O_MT + 20;      // O_MT: ce_math.h coefficient table
    // S = A^T Dy A on the matrix cores: NTILE column tiles of 16, row panels of A-hat staged with pitch LDP (= 16 mod 32 doubles: the
    // two row groups of a 32-lane LDS pass fall 128 bytes apart).  The G region holds at least one panel of 4 rows.
    static constexpr int NTILE = (NPg + 15) / 16;
    static constexpr int LDP = (16 * NTILE) % 32 == 16 ? 16 * NTILE : 16 * NTILE + 16;
    static_assert(NTILE <= NWARP && LDP >= NPa, "one 16-row strip of S per wave; a panel row holds a whole row tile");
    static_assert(T1 % 2 == 0 && T2 % 2 == 0 && TG % 2 == 0, "segments must be even for 16-byte LDS reads");
    static_assert(CHT <= 16 && CHA <= 16 && CHG <= 16, "DPP butterflies stay inside a row of 16 lanes");
};

// The launch geometry of one variant as plain numbers, for the host's planning table (ce_plan.h builds one per row of ce_variants.h)
struct F2Geom { int CHT, T1, CHA, T2, CHG, TG, NTH, MP, NPa, NPg, NP, VP, O_G, LDP; };
template <int CHT, int T1, int CHA, int T2, int CHG, int TG, int NTH>
constexpr F2Geom f2_geom() { using L = F2<CHT, T1, CHA, T2, CHG, TG, NTH / 64>; return {CHT, T1, CHA, T2, CHG, TG, NTH, L::MP, L::NPa, L::NPg, L::NP, L::VP, L::O_G, L::LDP}; }
// leading dimension of G in LDS: smallest even ld >= NPg for which the 16 lanes of an LDS group (CHG segments x 16/CHG rows)
// read 16 distinct 16-byte bank groups with ds_read_b128
__host__ __device__ inline int f2_pick_ldg(int CHG, int TG) {
    const int NPg = CHG * TG;
    for (int ld = NPg; ld < NPg + 64; ld += 2) {
        bool used[16] = {false}; bool ok = true;
        for (int lane = 0; lane < 16 && ok; lane++) {
            const int jg = lane / CHG, cg = lane % CHG;
            const int g = ((jg * ld + TG * cg) / 2) % 16;
            if (used[g]) ok = false; used[g] = true;
        }
        if (ok) return ld;
    }
    return NPg;
}
// whether a template fits the tiles of variant g of k_fwd2; then also ldg and the bytes of the kernel's dynamic LDS without the Anderson-acceleration tail
// (5 VP more doubles).  The carve: F2's fixed part up to O_G, the SOC row info (2 int arrays = MP doubles), the G region (k_fwd2's gsz), the PSD / triple
// scratch, P-hat g_x (has_p: the quadratic-objective kind)
__host__ __device__ inline bool f2_fits(const DevT &T, const F2Geom &g, bool has_p, int *ldg, size_t *bytes) {
    if ((T.n + 2) * g.CHT > g.NTH || T.m * g.CHA > g.NTH || T.n * g.CHG > g.NTH) return false;   // two extra column groups carry phi
    if (T.m > g.MP || T.n > g.NPa || T.n > g.NPg || T.n + T.m + 1 > g.NTH) return false;
    if (T.maxq > SOC_SMALL && T.nq > g.NP) return false;
    *ldg = f2_pick_ldg(g.CHG, g.TG);
    if ((size_t)T.n * *ldg < (size_t)g.NPa) return false;
    size_t gsz = (size_t)T.n * *ldg;                                    // G itself, one 4-row panel of the S formation, the exchange buffers of the blocked inversion
    if (gsz < (size_t)4 * g.LDP) gsz = (size_t)4 * g.LDP;
    if (gsz < (size_t)16 * g.NP) gsz = (size_t)16 * g.NP;
    *bytes = ((size_t)g.O_G + g.MP + gsz + fwd_cone_scratch_doubles(T.ns, T.maxs, T.nep + T.np) + (has_p ? g.NP : 0)) * 8;
    return true;
}
