// ce_plan.h -- the launch plan as a host unit: which kernel family and variant serves a template, with how much LDS, decided from the template's sizes, the
// rows of ce_variants.h, the footprint headers (ce_lds_*.h, ce_ns_layout.h) and the environment switches alone.  No HIP call and no HIP include: plain C++17
// apart from the footprints' __host__ __device__ qualifiers, so it compiles with g++ -D__host__= -D__device__= (tests/test_plan_host.py) as it does inside
// cone_engine.hip, which keeps the HIP half (device buffers, upload, launches).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "cone_engine.h"
#include "ce_devt.h"
#include "ce_variants.h"

namespace {
#include "ce_lds_common.h"
#include "ce_lds_fwd2.h"
#include "ce_lds_fwd_rt.h"
#include "ce_lds_fwd_generic.h"
#include "ce_lds_bwd_generic.h"
#include "ce_lds_bwd_rt.h"
#include "ce_ns_layout.h"
#include "ce_lds_psd_mfma.h"
#include "ce_lds_sa_fwd.h"
#include "ce_lds_sa_lsqr.h"
thread_local std::string g_err;      // ce_last_error

// The kernel family of each direction; the values are the numbers ce_get_plan / ce_get_launch_info report and the residency mode the size-generic launchers take
enum FwdMode { FWD_GEN_LDS = 0, FWD_GEN_G_GLOBAL = 1, FWD_GEN_GLOBAL = 2, FWD_RT = 3, FWD_V2 = 4 };      // k_forward (everything in LDS | A in LDS, G global | both global), k_forward_rt, k_fwd2
enum BwdMode { BWD_GEN_LDS = 0, BWD_GEN_K_GLOBAL = 1, BWD_GEN_GLOBAL = 2, BWD_RT = 3 };                  // k_backward (as forward, K for G), k_backward_rt
// The launch plan of a template: which kernel family and variant serves each direction, and with how much LDS.  Decided by plan_engine from the
// template's sizes and the environment switches alone (no HIP call); read by the launch paths, ce_get_plan and ce_get_launch_info.
struct CePlan {
    int fwd_mode = FWD_GEN_LDS; size_t fwd_lds = 0;
    int rt_variant = -1, rt_lda = 0;               // row of CE_RT_VARIANTS (-1: none fits)
    int f2_variant = -1, f2_ldg = 0;               // row of CE_F2_VARIANTS
    bool wl = false;                               // k_fwd2: rows packed so that cones are wave-local
    bool aa_ok = false;                            // k_fwd2: the launch carries the LDS for the Anderson-acceleration vectors
    bool qp_native = false;                        // the quadratic objective runs inside k_fwd2 and k_backward_rt
    int f2_neumann = 1, gen_blocked_f = 0, gen_blocked_b = 0;      // (copied into DevT: what the kernels read)
    int bwd_mode = BWD_GEN_LDS; size_t bwd_lds = 0; int nkcap = 0, ldk = 0;
    int brt_variant = -1;                          // row of CE_BRT_VARIANTS: the template's worst-case tile
    // two-tile plan of the register-tiled adjoint: a smaller tile serves the instances it holds, the worst-case tile re-runs the ones it flagged
    bool two_tile = false; int fast_forced = -1;
    int ns_variant = -1; size_t ns_lds = 0;        // row of CE_NS_VARIANTS: search-free null-space adjoint (-1: not applicable)
    int qp_ns_variant = -1; size_t qp_ns_lds = 0;  // row of CE_NS_VARIANTS with the QP footprint: forward derivative and refinement of a qp_native template (-1: none)
    int tri_ns_variant = -1; size_t tri_ns_lds = 0;      // row of CE_NS_VARIANTS with the TRI footprint: forward derivative and refinement of a template with exponential / power triples (-1: none)
    int psd_ns_variant = -1; size_t psd_ns_lds = 0;      // row of CE_NS_VARIANTS with the PSD footprint: the opt-in forward derivative and refinement of a template with PSD blocks (ce_jvp_psd, ce_refine_psd; -1: none)
    int psd_tri_ns_variant = -1; size_t psd_tri_ns_lds = 0;      // row of CE_NS_VARIANTS with both kinds' segments: the opt-in modes of a template with PSD blocks AND triples (ce_jvp_psd_tri, ...; -1: none)
};

#ifdef CE_TIMING
static constexpr size_t LDS_LIMIT = 160 * 1024 - 512;   // debug build: room for the static time-stamp array
#else
static constexpr size_t LDS_LIMIT = 160 * 1024;
#endif

// Planning tables: one entry per row of ce_variants.h, in the list's order (the variant index is the position)
struct F2Row { F2Geom g; bool wl, qp; };
struct RtRow { int CH1, T1, TG, CH2, T2, VP; };
struct BrtRow { int TI, TJ, TH, BGR; bool psd; };
struct NsRow { int NTILE, NTHR; };
struct SaFwdRow { int RP, NTH; bool cidx, tri; };
struct SaLsqrRow { int RP; bool psd, tri, lsmr, fwd; };
#define X(V, CHT, T1, CHA, T2, CHG, TG, NTH, WL, QP) {f2_geom<CHT, T1, CHA, T2, CHG, TG, NTH>(), WL != 0, QP != 0},
static const F2Row F2_ROWS[] = {CE_F2_VARIANTS(X)};
#undef X
#define X(V, CH1, T1, TG, CH2, T2, VP, WPE) {CH1, T1, TG, CH2, T2, VP},
static const RtRow RT_ROWS[] = {CE_RT_VARIANTS(X)};
#undef X
#define X(V, TI, TJ, TH, BGR, PSD) {TI, TJ, TH, BGR, PSD != 0},
static const BrtRow BRT_ROWS[] = {CE_BRT_VARIANTS(X)};
#undef X
#define X(V, NTILE, NTHR) {NTILE, NTHR},
static const NsRow NS_ROWS[] = {CE_NS_VARIANTS(X)};
#undef X
#define X(V, RP, NTH, CIDX, HTRI) {RP, NTH, CIDX != 0, HTRI != 0},
static const SaFwdRow SA_FWD_ROWS[] = {CE_SA_FWD_VARIANTS(X)};
#undef X
#define X(V, RP, HPSD, HTRI, LSMR, FWD) {RP, HPSD != 0, HTRI != 0, LSMR != 0, FWD != 0},
static const SaLsqrRow SA_LSQR_ROWS[] = {CE_SA_LSQR_VARIANTS(X)};
#undef X
template <int N> constexpr bool rows_in_order(const int (&v)[N]) { for (int i = 0; i < N; i++) if (v[i] != i) return false; return true; }
#define X(V, ...) V,
static_assert(rows_in_order({CE_F2_VARIANTS(X)}) && rows_in_order({CE_RT_VARIANTS(X)}) && rows_in_order({CE_BRT_VARIANTS(X)}) && rows_in_order({CE_NS_VARIANTS(X)}) &&
              rows_in_order({CE_SA_FWD_VARIANTS(X)}) && rows_in_order({CE_SA_LSQR_VARIANTS(X)}),
              "ce_variants.h: a row's index is its position in its list");
#undef X
}  // namespace

static size_t brt_lds_bytes(const DevT &T, int v) { return bwd_rt_lds_bytes(T, BRT_ROWS[v].TI, BRT_ROWS[v].TJ, BRT_ROWS[v].BGR); }
// a first tile of the two-tile plan must hold the template and differ from the worst-case tile in TI / TJ alone: a tile with another H tile or row-residue
// count sums in another order, and its gradients would differ in the last bits from the single-tile plan's
static bool brt_tile_holds(const DevT &T, int v) { return T.n <= BGC * BRT_ROWS[v].TH && brt_lds_bytes(T, v) <= LDS_LIMIT; }
static bool brt_first_tile_ok(const DevT &T, int v, int worst) { return BRT_ROWS[v].TH == BRT_ROWS[worst].TH && BRT_ROWS[v].BGR == BRT_ROWS[worst].BGR && brt_tile_holds(T, v); }

// the re-solve behind ce_vjp / ce_jvp: the LSQR vectors of one instance (CSR / CSC products: per-instance values) fit LDS.  psd_first: the first row behind the
// second-order cones (DevT::eoff when the template has no PSD block)
static bool resolve_lds_fits(const DevT &T, int psd_first) {
    return sa_lsqr_lds_doubles(T.n, T.m, T.nq, T.ns, T.maxs, 0, psd_first, T.nep + T.np) * 8 <= LDS_LIMIT;
}
// k_backward_ns: the first row of CE_NS_VARIANTS whose tiles hold the reduced system (4 ceil(n / 4) + 1 columns) and whose layout (with P: the dense P on top) fits LDS;
// -1: none.  *lds: its footprint
static int ns_first_fit(const DevT &T, bool qp, size_t *lds, int ntri = 0, int psdrows = 0) {      // (ntri > 0: the layout's TRI mode, the triples' W and lambda on top;
    for (int v = 0; v < (int)std::size(NS_ROWS); v++) {                                               //  psdrows > 0: its PSD mode, the rows the T.ns blocks own together)
        const size_t by = (psdrows > 0 && ntri > 0) ? bwd_ns_psd_tri_lds_bytes_of(T.n, T.m, T.nq, ntri, T.ns, T.maxs, psdrows, NS_ROWS[v].NTILE, NS_ROWS[v].NTHR)      // (both counts: both kinds' segments)
                        : psdrows > 0 ? bwd_ns_psd_lds_bytes_of(T.n, T.m, T.nq, T.ns, T.maxs, psdrows, NS_ROWS[v].NTILE, NS_ROWS[v].NTHR)
                        : ntri > 0 ? bwd_ns_tri_lds_bytes_of(T.n, T.m, T.nq, ntri, NS_ROWS[v].NTILE, NS_ROWS[v].NTHR)
                        : qp ? bwd_ns_qp_lds_bytes_of(T.n, T.m, T.nq, NS_ROWS[v].NTILE, NS_ROWS[v].NTHR) : bwd_ns_lds_bytes_of(T.n, T.m, T.nq, NS_ROWS[v].NTILE, NS_ROWS[v].NTHR);
        if (4 * ((T.n + 3) / 4) + 1 <= 16 * NS_ROWS[v].NTILE && by <= LDS_LIMIT) { *lds = by; return v; }
    }
    return -1;
}

// Row order for k_fwd2's wave-local cone exchange (ce_forward_v2.h, WL): the rows of one wave in the (i2, c2) row layout form a
// window of W = 64 / CHA rows, and no cone may straddle two windows.  Zero-cone rows stay first (the kernel tells them by i < z);
// then the SOC blocks in template order, each pushed to the next window when it would straddle, the gap filled with nonnegative
// rows (which are interchangeable: they count as cones of dimension 1); the remaining nonnegative rows go last.  Exact fit only
// (no padding rows: they would change the size of the embedding and with it the iterates); returns false when that fails.
static bool pack_rows(const ce_template *tpl, int W, std::vector<int> &korig, std::vector<int> &k_rowcone, std::vector<int> &k_qoff) {
    const int z = tpl->z, l = tpl->l, m = tpl->m;
    if (tpl->ns > 0 || tpl->nep + tpl->np > 0) return false;
    for (int c = 0; c < tpl->nq; c++) if (tpl->q[c] > W) return false;
    korig.clear(); k_rowcone.assign(m, -1); k_qoff.clear();
    for (int i = 0; i < z; i++) korig.push_back(i);
    int next_single = z, singles_left = l, orig = z + l;
    auto place_single = [&]() { k_rowcone[korig.size()] = (int)k_qoff.size(); k_qoff.push_back((int)korig.size()); korig.push_back(next_single++); singles_left--; };
    for (int c = 0; c < tpl->nq; c++) {
        const int d = tpl->q[c];
        const int used = (int)korig.size() % W;
        if (used + d > W) {
            const int need = W - used;
            if (singles_left < need) return false;
            for (int k = 0; k < need; k++) place_single();
        }
        k_qoff.push_back((int)korig.size());
        for (int k = 0; k < d; k++) { k_rowcone[korig.size()] = (int)k_qoff.size() - 1; korig.push_back(orig++); }
    }
    while (singles_left > 0) place_single();
    k_qoff.push_back((int)korig.size());
    return (int)korig.size() == m;
}


// What the plan reads of a (validated) template: the sizes of T (not its device pointers, nor the three flags copied from the plan) and, as the one walk over
// the cones gives them, the first row of every second-order cone and PSD block (qoff[nq], soff[ns]: the row behind the last; soff[0] is the first row behind the
// second-order cones, m when nothing follows; exponential / power triples follow the PSD blocks)
static void plan_sizes(const ce_template *tpl, DevT &T, std::vector<int> &qoff, std::vector<int> &soff) {
    T.n = tpl->n; T.m = tpl->m; T.nnz_aug = tpl->nnz_aug; T.nnzA = tpl->indptr[tpl->n]; T.z = tpl->z; T.l = tpl->l; T.nq = tpl->nq;
    T.lda = tpl->n | 1; T.ldg = tpl->n | 1; T.maxq = 0;     // odd leading dimension: conflict-free ds_read_b64 down a column of rows
    qoff.assign(tpl->nq + 1, 0); soff.assign(tpl->ns + 1, 0);
    int r = tpl->z + tpl->l;
    for (int c = 0; c < tpl->nq; c++) { qoff[c] = r; T.maxq = std::max(T.maxq, tpl->q[c]); r += tpl->q[c]; }
    qoff[tpl->nq] = r;
    T.ns = tpl->ns; T.maxs = 0;
    for (int c = 0; c < tpl->ns; c++) { soff[c] = r; T.maxs = std::max(T.maxs, tpl->s[c]); r += tpl->s[c] * (tpl->s[c] + 1) / 2; }
    soff[tpl->ns] = r;
    T.nep = tpl->nep; T.eoff = r; T.np = tpl->np;
}
// The shared-A kernels' split of the A part: the rows with several entries (the "dense" rows), in row order ...
static std::vector<int> dense_rows(const ce_template *tpl) {
    std::vector<int> cnt(tpl->m, 0), rows;
    for (int k = 0; k < tpl->indptr[tpl->n]; k++) cnt[tpl->indices[k]]++;
    for (int i = 0; i < tpl->m; i++) if (cnt[i] >= 2) rows.push_back(i);
    return rows;
}
// ... and their count padded to 16 / 32 / 64 (*r: the count), or 0 (and *r = 0) when there are more than 64: no split, CSR / CSC products
static int split_RP(int dense, int *r) {
    *r = dense > 64 ? 0 : dense;
    return dense > 64 ? 0 : (dense <= 16 ? 16 : (dense <= 32 ? 32 : 64));
}

// the environment switches of the plan (A/B switches for benchmarking and the tests), read once per ce_create
struct PlanEnv { bool force_generic, fwd_rt, fwd_generic, wl_off, neumann_off, gen_blocked_off, two_tile_off, ns_off; int fast_forced; };
static PlanEnv read_plan_env() {
    const auto is = [](const char *name, const char *val) { const char *e = getenv(name); return e && !strcmp(e, val); };
    const auto zero = [](const char *name) { const char *e = getenv(name); return e && atoi(e) == 0; };
    PlanEnv E;
    E.force_generic = getenv("CE_FORCE_GENERIC") != nullptr;
    E.fwd_rt = is("CE_FWD", "rt"); E.fwd_generic = is("CE_FWD", "generic");      // (default "v2": k_fwd2 when it fits)
    E.wl_off = is("CE_WL", "0");                                                 // keep the template's row order
    E.neumann_off = zero("CE_F2_NEUMANN");
    E.gen_blocked_off = is("CE_GEN_BLOCKED", "0");                               // the unblocked elimination of the size-generic backward kernel
    E.two_tile_off = is("CE_BWD_TWO_TILE", "0");
    const char *fv = getenv("CE_BWD_FAST_VARIANT"); E.fast_forced = fv ? atoi(fv) : -1;      // forces the first tile of the two-tile plan
    E.ns_off = zero("CE_BWD_NS");
    return E;
}
// residency of the size-generic forward kernel: mode 0 = everything in LDS, 1 = A in LDS / G in global memory, 2 = both in global memory
// (modes 1, 2: the blocked inversion needs its column panel in LDS; templates where that does not fit keep the unblocked loop)
static bool plan_fwd_generic(const DevT &T, CePlan &P) {
    if (fwd_lds_bytes(T, true, true) <= LDS_LIMIT) P.fwd_mode = FWD_GEN_LDS;
    else if (fwd_lds_bytes(T, true, false) <= LDS_LIMIT) P.fwd_mode = FWD_GEN_G_GLOBAL;
    else if (fwd_lds_bytes(T, false, false) <= LDS_LIMIT) P.fwd_mode = FWD_GEN_GLOBAL;
    else return false;
    P.gen_blocked_f = (P.fwd_mode != FWD_GEN_LDS && fwd_lds_bytes(T, P.fwd_mode != FWD_GEN_GLOBAL, false, true) <= LDS_LIMIT) ? 1 : 0;
    P.fwd_lds = fwd_lds_bytes(T, P.fwd_mode != FWD_GEN_GLOBAL, P.fwd_mode == FWD_GEN_LDS, P.gen_blocked_f != 0);
    return true;
}
// The plan of a template: every family takes the FIRST row of its list that is instantiated for the template's kind and fits.  No HIP call.
static int plan_engine(const ce_template *tpl, const DevT &T, int nnz_p, const PlanEnv &E, CePlan &P) {
    const bool plain = T.ns == 0 && T.nep + T.np == 0;
    if (!plan_fwd_generic(T, P)) { g_err = "instance vectors do not fit LDS"; return CE_E_TOO_LARGE; }
    if (!E.force_generic && plain) {      // (k_forward_rt: zero / nonnegative / second-order cones only)
        for (int v = 0; v < (int)std::size(RT_ROWS); v++) {
            const RtRow &R = RT_ROWS[v]; int ld; size_t by;
            if (rt_fits(T, R.CH1, R.T1, R.TG, R.CH2, R.T2, R.VP, &ld, &by) && by <= LDS_LIMIT) { P.rt_variant = v; P.fwd_lds = by; P.fwd_mode = FWD_RT; P.rt_lda = ld; break; }
        }
    }
    if (!E.force_generic && !E.fwd_rt && !E.fwd_generic) {
        const bool has_p = nnz_p > 0 && plain;     // P inside the kernels: plain cones only (else: epigraph form upstream)
        for (int v = 0; v < (int)std::size(F2_ROWS); v++) {
            const F2Row &R = F2_ROWS[v]; int ldg; size_t by;
            if ((has_p && !R.qp) || !f2_fits(T, R.g, has_p, &ldg, &by) || by > LDS_LIMIT) continue;
            P.f2_variant = v; P.f2_ldg = ldg; P.fwd_lds = by; P.fwd_mode = FWD_V2; P.qp_native = has_p;
            // kernel row order: packed for the wave-local cone exchange when the template allows it (plain cones, linear objective)
            std::vector<int> ko, krc, kq;
            P.wl = !has_p && R.wl && !E.wl_off && pack_rows(tpl, 64 / R.g.CHA, ko, krc, kq);
            // five more vectors (w_prev, x_prev, f_prev, f_save, x_save) when they fit: Anderson acceleration available
            if (by + 5 * (size_t)R.g.VP * 8 <= LDS_LIMIT) { P.fwd_lds = by + 5 * (size_t)R.g.VP * 8; P.aa_ok = true; }
            break;
        }
    }
    if (E.fwd_generic && P.fwd_mode == FWD_RT) { P.rt_variant = -1; plan_fwd_generic(T, P); }      // forced generic kernel
    P.nkcap = T.n + std::min(T.m, T.n);
    P.ldk = (P.nkcap + 1) | 1;
    if (bwd_lds_bytes(T, true, true, P.nkcap, P.ldk) <= LDS_LIMIT) P.bwd_mode = BWD_GEN_LDS;
    else if (bwd_lds_bytes(T, true, false, P.nkcap, P.ldk) <= LDS_LIMIT) P.bwd_mode = BWD_GEN_K_GLOBAL;
    else if (bwd_lds_bytes(T, false, false, P.nkcap, P.ldk) <= LDS_LIMIT) P.bwd_mode = BWD_GEN_GLOBAL;
    else { g_err = "instance vectors do not fit LDS"; return CE_E_TOO_LARGE; }
    P.f2_neumann = E.neumann_off ? 0 : 1;
    P.gen_blocked_b = (!E.gen_blocked_off && P.bwd_mode != BWD_GEN_LDS && bwd_lds_bytes(T, P.bwd_mode != BWD_GEN_GLOBAL, false, P.nkcap, P.ldk, true) <= LDS_LIMIT) ? 1 : 0;
    P.bwd_lds = bwd_lds_bytes(T, P.bwd_mode != BWD_GEN_GLOBAL, P.bwd_mode == BWD_GEN_LDS, P.nkcap, P.ldk, P.gen_blocked_b != 0);
    if (!E.force_generic) {
        for (int v = 0; v < (int)std::size(BRT_ROWS); v++) {
            const BrtRow &R = BRT_ROWS[v];
            if ((!plain && !R.psd) || P.nkcap > BGC * R.TJ - 1 || P.nkcap > R.BGR * R.TI || !brt_tile_holds(T, v)) continue;
            P.brt_variant = v; P.bwd_mode = BWD_RT; P.bwd_lds = brt_lds_bytes(T, v); break;
        }
        // Two-tile plan.  The tile above holds the template's WORST case (NK <= n + min(m, n): every row active); the systems of a batch are usually much
        // smaller (metric configuration: NK = 61 .. 81 of 111) and on the worst-case tile most of every pivot's broadcast and rank-1 update runs over
        // empty column slots.  ce_vjp therefore serves the batch on the smallest tile that held the LARGEST system of the previous call (+ margin) and
        // re-runs the instances that tile flags (adj 2) on the worst-case tile, which exits at once for everybody else.  A retry is expensive however few
        // there are (its launch lasts as long as one instance takes on an idle device, ~0.09 ms at the metric configuration: profiles/r04/e_ab_bwd_two_tile.log),
        // hence the history instead of an a-priori guess (config 3: half of the instances have a fully active cone, NK up to 170 of 200 -- no smaller tile).
        // CE_BWD_TWO_TILE=0 disables; CE_BWD_FAST_VARIANT=v forces the first tile (tests).  Without a first tile (worst case v4 or v5) the plan has nothing to offer.
        P.fast_forced = E.fast_forced;
        bool first_tile = P.brt_variant > 0 && P.fast_forced >= 0 && P.fast_forced < P.brt_variant;
        for (int v = 0; v < P.brt_variant && !first_tile; v++) first_tile = brt_first_tile_ok(T, v, P.brt_variant);
        P.two_tile = P.bwd_mode == BWD_RT && plain && nnz_p == 0 && first_tile && !E.two_tile_off;
    }
    // Search-free null-space adjoint (ce_backward_ns.h): plain cones, linear objective, 4 ceil(n / 4) + 1 columns in the variant's tiles.  It serves ce_vjp calls
    // whose LSQR re-solve is armed (rank-deficient instances are detected, flagged and handed to LSQR, not resolved by the elimination).  CE_BWD_NS=0 disables.
    if (plain && nnz_p == 0 && !E.ns_off && !E.force_generic) P.ns_variant = ns_first_fit(T, false, &P.ns_lds);
    if (P.qp_native && P.bwd_mode != BWD_RT) P.qp_native = false;      // the adjoint with P lives in the register-tiled backward kernel
    // The same elimination with P inside (k_backward_ns<..., QP>): the forward derivative and the refinement of a qp_native template, planned on its own
    // footprint (the dense P on top).  ns_variant stays -1 for such a template: its adjoint keeps k_backward_rt.
    if (P.qp_native && !E.ns_off) P.qp_ns_variant = ns_first_fit(T, true, &P.qp_ns_lds);
    // And with exponential / power triples beside the plain cones (k_backward_ns<..., TRI>): the forward derivative and the refinement, linear objective, no PSD
    // block, planned on the TRI footprint -- when the LSQR vectors of the re-solve behind ce_jvp fit LDS too (with no PSD block, v = y - s is kept for every row in
    // front of the triples).  ns_variant stays -1: the adjoint of such a template keeps k_backward_rt.
    if (T.ns == 0 && T.nep + T.np > 0 && nnz_p == 0 && !E.ns_off && !E.force_generic && resolve_lds_fits(T, T.eoff))
        P.tri_ns_variant = ns_first_fit(T, false, &P.tri_ns_lds, T.nep + T.np);
    // And with PSD blocks beside the plain cones (k_backward_ns<..., PSD>): the forward derivative and the refinement behind entry points of their own (ce_jvp_psd,
    // ce_refine_psd), linear objective, no triple, planned on the PSD footprint -- when the LSQR vectors of the re-solve fit LDS too.  psd_first: the blocks' first
    // row, qoff[nq] (plan_sizes: the PSD rows end at T.eoff, and nothing follows them here).  Every other field keeps its value: ce_jvp / ce_refine still refuse.
    if (T.ns > 0 && T.nep + T.np == 0 && nnz_p == 0 && !E.ns_off && !E.force_generic) {
        int psdrows = 0;
        for (int c = 0; c < tpl->ns; c++) psdrows += tpl->s[c] * (tpl->s[c] + 1) / 2;
        if (resolve_lds_fits(T, T.eoff - psdrows)) P.psd_ns_variant = ns_first_fit(T, false, &P.psd_ns_lds, 0, psdrows);
    }
    // And with BOTH, PSD blocks and triples beside the plain cones (k_backward_ns<..., TRI, ..., PSD>): the forward derivative, the refinement and the two
    // many-modes behind entry points of their own (ce_jvp_psd_tri, ce_refine_psd_tri, ce_vjp_psd_tri_many, ce_jvp_psd_tri_many), linear objective, planned on the
    // footprint with both kinds' segments -- when the LSQR vectors of the re-solve fit LDS too.  The four fields above stay -1 for such a template.
    if (T.ns > 0 && T.nep + T.np > 0 && nnz_p == 0 && !E.ns_off && !E.force_generic) {
        int psdrows = 0;
        for (int c = 0; c < tpl->ns; c++) psdrows += tpl->s[c] * (tpl->s[c] + 1) / 2;
        if (resolve_lds_fits(T, T.eoff - psdrows)) P.psd_tri_ns_variant = ns_first_fit(T, false, &P.psd_tri_ns_lds, T.nep + T.np, psdrows);
    }
    return CE_OK;
}


// Shared-A kernels: the row of the family's list (ce_variants.h) that serves a call and the LDS of its launch, from the template's sizes and the switches, which
// are read HERE, at every call.  No HIP call.  lds == 0: the vectors of one instance do not fit LDS.
struct SaFwdSel { int row = -1; size_t lds = 0; int aa_w_lds = 0; };
struct SaLsqrSel { int row = -1; size_t lds = 0; int RP = 0, a_lds = 0; };
static int env_int(const char *name, int dflt) { const char *e = getenv(name); return e ? atoi(e) : dflt; }
static SaFwdSel sa_fwd_select(const DevT &T, int r, int RP, bool aa) {
    SaFwdSel out;
    const bool tri = T.nep + T.np > 0;
    // 512 threads per instance when the iterates of one instance leave room for a single workgroup per CU anyway (CE_SA_NT=256 / 512 forces);
    // that instantiation also keeps the template's index arrays in LDS when they fit (CE_SA_CIDX=0 disables)
    int nth = 256;
    if (T.ns == 0 && sa_fwd_lds_doubles(T.n, T.m, T.nq, T.ns, T.maxs, RP, 256, T.nep + T.np) * 8 > LDS_LIMIT / 2) nth = 512;
    { const int v = env_int("CE_SA_NT", 0); if (v == 256 || (v == 512 && T.ns == 0)) nth = v; }
    size_t lds = sa_fwd_lds_doubles(T.n, T.m, T.nq, T.ns, T.maxs, RP, nth, T.nep + T.np) * 8;
    if (lds > LDS_LIMIT) return out;
    bool cidx = false;
    if (nth == 512) {
        const size_t with = lds + sa_fwd_cidx_doubles(T.n, T.m, T.nq, r, T.m) * 8;      // (at most m single-entry rows)
        if (with <= LDS_LIMIT && env_int("CE_SA_CIDX", 1) != 0) { cidx = true; lds = with; }
    }
    if (aa) {
        // the input of the last iteration in LDS when that does not cost a workgroup per CU (config 4: 68.7 + 3.5 KB, still two per CU)
        const size_t l = (size_t)T.n + T.m + 1, lp = l + (l & 1), per_cu = nth == 256 ? LDS_LIMIT / 2 : LDS_LIMIT;
        if (lds + lp * 8 <= per_cu || (lds > LDS_LIMIT / 2 && lds + lp * 8 <= LDS_LIMIT)) { out.aa_w_lds = 1; lds += lp * 8; }
    }
    // (the rows without CIDX carry the triples' code whatever the template)
    for (int v = 0; v < (int)(sizeof(SA_FWD_ROWS) / sizeof(SA_FWD_ROWS[0])); v++) {
        const SaFwdRow &R = SA_FWD_ROWS[v];
        if (R.RP == RP && R.NTH == nth && R.cidx == cidx && R.tri == (tri || !cidx)) { out.row = v; break; }
    }
    out.lds = lds;
    return out;
}
// per_inst: every instance has its own A values;  listed: the launch walks a re-solve list;  fwd: the forward derivative
static SaLsqrSel sa_lsqr_select(const DevT &T, int sp_RP, int psd_first, int lsqr_variant, bool per_inst, bool listed, bool fwd) {
    SaLsqrSel out;
    const bool tri = T.nep + T.np > 0, psd = T.ns > 0;
    // products through the singleton / dense-row split when the template has one (CE_SA_SPLIT=0: CSR / CSC products)
    int RP = env_int("CE_SA_SPLIT", 1) == 0 ? 0 : sp_RP;
    if (per_inst) RP = 0;      // the split's dense rows are ONE matrix (instance 0's values); per-instance values go through the CSR / CSC products
    const bool lsmr = lsqr_variant == 1 && !listed && !fwd;      // (the re-solve list of ce_vjp stays diffcp's default, LSQR)
    if (RP > 0 && sa_lsqr_lds_doubles(T.n, T.m, T.nq, T.ns, T.maxs, RP, psd_first, T.nep + T.np, lsmr) * 8 > LDS_LIMIT) RP = 0;
    size_t lds = sa_lsqr_lds_doubles(T.n, T.m, T.nq, T.ns, T.maxs, RP, psd_first, T.nep + T.np, lsmr) * 8;
    if (lds > LDS_LIMIT) return out;
    // per-instance A: staged dense in LDS when it fits behind the vectors with three workgroups per CU to spare (CE_LSQR_A_LDS=0 disables)
    if (per_inst && RP == 0) {
        const size_t with = lds + 8 + sizeof(double) * (size_t)T.m * T.n;
        if (env_int("CE_LSQR_A_LDS", 1) != 0 && with <= LDS_LIMIT / 3) { out.a_lds = 1; lds = with; }
    }
    { const size_t want = (size_t)env_int("CE_SA_LSQR_PADLDS", 0) * 1024; if (want > lds && want <= LDS_LIMIT) lds = want; }      // (residency experiment: workgroups per CU)
    // the leanest row that has the code the template's cones need: plain cones / PSD without triples run instantiations without the other cones' code
    // (CE_SA_LSQR_SPEC=0: the adjoint runs the general kernel)
    const bool spec = fwd || env_int("CE_SA_LSQR_SPEC", 1) != 0;
    for (int v = 0; v < (int)(sizeof(SA_LSQR_ROWS) / sizeof(SA_LSQR_ROWS[0])); v++) {
        const SaLsqrRow &R = SA_LSQR_ROWS[v];
        if (R.RP != RP || R.lsmr != lsmr || R.fwd != fwd || (psd && !R.psd) || (tri && !R.tri) || (!spec && !(R.psd && R.tri))) continue;
        if (out.row < 0 || R.psd + R.tri < SA_LSQR_ROWS[out.row].psd + SA_LSQR_ROWS[out.row].tri) out.row = v;
    }
    out.lds = lds; out.RP = RP;
    return out;
}
