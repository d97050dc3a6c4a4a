// cone_engine.hip -- MI355X (gfx950 / CDNA4) batched cone-program solve + differentiate engine.
//
// One problem instance per 256-thread workgroup (4 wave64).  The instance's data (dense A in solver
// form, the explicit inverse G of the reduced KKT matrix, all iterates) live in LDS for the whole
// solve: HBM is touched once per instance on the way in (coalesced batch-major value rows) and once
// on the way out.  fp64 throughout (the reference returns float64, diffcp_if.py:374-375).
//
// Forward  : homogeneous self-dual embedding + Douglas-Rachford splitting (SCS 3 algorithm, restated
//            in oracle/cone_oracle.c which this file must agree with), with the per-iteration KKT
//            solve done as  t = rho_x w_x - A^T w_y ;  p_x = G t ;  p_y = w_y + Dy (A p_x)  where
//            G = (rho_x I + A^T Dy A)^{-1} is formed once per (re)scaling by in-LDS Gauss-Jordan.
//            Triangular solves are latency-bound on a GPU; an explicit inverse turns them into matvecs.
// Backward : diffcp's adjoint  M^T r = dz  solved DIRECTLY: the homogeneous embedding makes M singular
//            along z, dA/db/dc are invariant to that null component, so r_tau is pinned to 0 and the
//            remaining (n+m) system is reduced, cone block by cone block, with the spectral structure
//            of DPi (eigenvalue 1 -> equality row, 0 -> eliminated, lambda in (0,1) -> Schur term) to a
//            symmetric saddle system of size n + #equality rows, solved by Gauss-Jordan with partial
//            pivoting in LDS.  See DESIGN.md section "Backward".
//
// Reference boundary mirrored: cvxpylayers/interfaces/diffcp_if.py:46-96,329-403.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <type_traits>
#include <utility>
#include <atomic>
#include <memory>
#include <vector>

#include "cone_engine.h"
#include "ce_types.h"
#include "ce_plan.h"           // the launch plan (host only): CePlan, plan_engine, the shared-A selectors, the footprints of every kernel family
#include "ce_lds_fwd_wave.h"   // k_fwd_wave (ce_solve_wave): served class, row and footprint -- beside the plan, not a field of it

namespace {
// the kernels this file launches itself; every other family is instantiated in its own translation unit (ce_tu_*.hip) and reached through the launchers of ce_types.h
#include "ce_const_a.h"        // k_ca_*
#include "ce_layout_kernels.h" // k_transpose, k_parammap*
}  // namespace
#ifndef BRT_HAS_PSD
#define BRT_HAS_PSD 1
#endif

// ================================================================================================
// host side
// ================================================================================================
#define HIPCHK(call)                                                                 \
    do {                                                                             \
        hipError_t e_ = (call);                                                      \
        if (e_ != hipSuccess) {                                                      \
            g_err = std::string(#call) + ": " + hipGetErrorString(e_);               \
            return CE_E_HIP;                                                         \
        }                                                                            \
    } while (0)

// ce_last_error for the entry points that live in a translation unit of their own (ce_tu_cone_proj.hip): g_err has internal linkage
void ce_set_last_error(const std::string &msg) { g_err = msg; }

// Device memory of the engine: move-only, freed with its owner.  reserve() only ever grows the buffer and does not keep its contents.
template <class T>
class DevBuf {
    T *p = nullptr; size_t cap = 0;      // (capacity in elements)
public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
    ~DevBuf() { if (p) hipFree(p); }
    T *get() const { return p; }
    size_t capacity() const { return cap; }
    hipError_t reserve(size_t count) {
        if (cap >= count) return hipSuccess;
        if (p) hipFree(p);
        p = nullptr; cap = 0;
        const hipError_t e = hipMalloc(&p, sizeof(T) * count);
        if (e == hipSuccess) cap = count;
        return e;
    }
    hipError_t upload(const T *src, size_t count) {
        const hipError_t e = reserve(count);
        return (e != hipSuccess || count == 0) ? e : hipMemcpy(p, src, sizeof(T) * count, hipMemcpyHostToDevice);
    }
    hipError_t upload(const std::vector<T> &v) { return upload(v.data(), v.size()); }
};

struct ce_engine {
    int device = 0;
    DevT T{};
    CePlan plan;
    std::vector<int> q, s;
    DevBuf<double> d_pw;
    DevBuf<int> d_rowidx, d_colidx, d_rowcone, d_qoff, d_soff, d_sord;
    // workspace
    DevBuf<double> wsA;          // batch-major copy of A_vals  [B][nnz_aug]
    DevBuf<double> wsdA;         // batch-major dA              [B][nnz_aug]
    DevBuf<double> gws;          // global residency fallback
    const double *retained_A = nullptr; int retained_B = 0;
    int wave_variant = -1; size_t wave_lds = 0;      // k_fwd_wave (ce_solve_wave): row of CE_WAVE_VARIANTS that serves the template (-1: none) and its dynamic LDS
    bool transient_solve = false;          // ce_set_transient_solve: ce_solve / ce_solve_qp leave retained_A and the dispatch history as they found them
    uintptr_t summary_host_checked = 0; char *summary_host_dev = nullptr;      // ce_status_summary: the last 64-byte line of host memory examined and its device alias (null: not mapped)
    DevBuf<int> d_idx_at, d_idx_ar, d_idx_b;       // k_fwd2: gather maps of the two register tiles of A and of b
    DevBuf<int> d_csc_ptr, d_csr_ptr, d_csr_col, d_csr_src;   // sparse structure of the A part (shared-A kernels)
    // split of the A part into singleton rows and sp_r <= 64 dense rows (ce_shared_a_ops.h); sp_RP == 0: more than 64 rows with several entries
    int sp_r = 0, sp_RP = 0;
    DevBuf<int> d_sp_drow, d_sp_srow_col, d_sp_scol_ptr, d_sp_scol_row, d_sp_rowslot, d_sp_sing_i;
    DevBuf<double> d_sp_sing_v, d_sp_AdT, d_sp_sval;
    DevBuf<int> d_bpos;          // [m] position of the row's b entry in the boundary's value order (-1: structurally zero): the tau column of the shared-A adjoint
    bool sa_fwd_attr = false, sa_lsqr_attr = false;      // MaxDynamicSharedMemorySize is per device: set once per engine (an engine is bound to one device, one caller thread)
    int last_sa_fwd = -1, last_sa_lsqr = -1;       // rows of CE_SA_FWD_VARIANTS / CE_SA_LSQR_VARIANTS the last such launch ran (-1: none yet; ce_get_plan)
    int lsqr_variant = 0;                          // 0: LSQR, 1: LSMR (ce_set_lsqr_variant; the calls that solve EVERY instance iteratively: ce_vjp_shared_a, ce_vjp_lsqr)
    DevBuf<int> d_summary; unsigned summary_next = 0;   // ce_status_summary staging (8 slots of 3 ints)
    DevBuf<double> d_dy0;        // ce_vjp_many with dy == NULL: one zero dy [B][m] that every cotangent reads
    DevBuf<double> d_rec;        // ce_vjp_many_params: the factor records [K][B][m + 1 + n] the adjoint leaves for k_param_grad
    const CeParamGradArgs *pg = nullptr;      // (ce_vjp_params -> ce_vjp_qp: the call in flight wants the parameter gradient, not the dA row)
    DevBuf<double> d_qT;       // batch-major copy of the objective values for the LSQR adjoint kernels (vjp_lsqr_launch)
    DevBuf<double> d_aa_ws;      // Anderson-acceleration history of the shared-A forward kernel ([B][4][lp])
    DevBuf<unsigned long long> d_psd_stats;        // CE_PSD_STATS=1: counters of the PSD projection (printed to stderr by ce_destroy)
    int psd_first = 0;           // first row of the first PSD block (m when the template has none)
    int wl_nq = 0; DevBuf<int> d_row_perm, d_k_rowcone, d_k_qoff;   // plan.wl: kernel row -> template row, and the cone layout in the kernel's row order
    // longest-first dispatch (ce_set_dispatch_history): workgroup -> instance order for the next solve of the same batch size, from this solve's iteration counts
    bool dispatch_history = false; DevBuf<int> d_order; int order_B = 0;
    DevBuf<int> d_iters2; int order_pending_B = 0; const int *last_status = nullptr;      // engine-owned copy of the last solve's iteration counts; last_status: the status vector of the solve whose order is pending
    DevBuf<int> d_iters_prev; int iters_prev_B = 0;      // the iteration counts of the call before (k_dispatch_order compares: is the history predictive?)
    // two-tile plan: the smaller tile is chosen from the LARGEST system of the previous call of the same batch size (nk_*: device maximum, copied to pinned memory behind the launch)
    int last_fast = -1;      // first tile of the last two-tile call (-1: none; ce_get_plan)
    DevBuf<int> d_nkmax; int *h_nkmax = nullptr; hipEvent_t nk_ev = nullptr; bool nk_pending = false, nk_have = false, nk_zeroed = false; int nk_last = 0, nk_B = 0;
    // re-solve of rank-deficient adjoint systems by LSQR (ce_set_adjoint_resolve): fix[0] = number of listed instances, fix[1 ...] = the instances the elimination
    // kernels flagged (appended on the device); diffcp's LSQR rule
    const double *call_q = nullptr; long call_sqk = 0, call_sqb = 0;      // (ce_vjp -> ce_vjp_qp: the objective values of the call in flight)
    bool resolve = true; DevBuf<int> d_fix; int fix_cap = 0, fix_par = 0; double rs_atol = 1e-8, rs_btol = 1e-8, rs_conlim = 1e8; int rs_iter_lim = 0;
    // quadratic objective
    int nnz_p = 0, p_tri = 0;
    std::vector<int> p_rows, p_cols;               // host copy of the P structure (entry -> (row, col))
    DevBuf<int> d_idx_p, d_pmap, d_prow, d_pcol;
    // profiling
    int prof = 0;      // bit w: launches of kind w (0 forward, 1 adjoint, 2 layout passes) are bracketed by HIP events
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[3];
    std::vector<hipEvent_t> ev_pool;
    // (pinned memory and events are released here, device memory by the DevBuf members; the caller has selected the engine's device)
    ~ce_engine() {
        if (h_nkmax) hipHostFree(h_nkmax);
        if (nk_ev) hipEventDestroy(nk_ev);
        for (auto &v : ev) for (auto &p : v) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
        for (auto &e : ev_pool) hipEventDestroy(e);
    }
};

// ---- ce_create = validate -> index -> plan -> upload
static int validate_template(const ce_template *tpl, ce_handle *out) {
    if (!tpl || !out || tpl->n <= 0 || tpl->m <= 0 || !tpl->indices || !tpl->indptr) { g_err = "bad template"; return CE_E_BADARG; }
    if (tpl->nep < 0 || tpl->np < 0 || (tpl->np > 0 && !tpl->p)) { g_err = "bad exponential / power cone description"; return CE_E_BADARG; }
    for (int i = 0; i < tpl->np; i++) if (!(fabs(tpl->p[i]) > 0.0 && fabs(tpl->p[i]) < 1.0)) { g_err = "power cone exponent must lie in (-1, 0) or (0, 1)"; return CE_E_BADARG; }
    int rows = tpl->z + tpl->l;
    for (int i = 0; i < tpl->nq; i++) { if (tpl->q[i] < 1) { g_err = "bad SOC dim"; return CE_E_BADARG; } rows += tpl->q[i]; }
    for (int i = 0; i < tpl->ns; i++) { if (tpl->s[i] < 1) { g_err = "bad PSD order"; return CE_E_BADARG; } rows += tpl->s[i] * (tpl->s[i] + 1) / 2; }
    rows += 3 * tpl->nep + 3 * tpl->np;
    if (rows != tpl->m) { g_err = "cone dims do not add up to m"; return CE_E_BADARG; }
    if (tpl->indptr[tpl->n + 1] != tpl->nnz_aug) { g_err = "indptr[n+1] != nnz_aug"; return CE_E_BADARG; }
    for (int k = tpl->indptr[0]; k < tpl->nnz_aug; k++) if (tpl->indices[k] < 0 || tpl->indices[k] >= tpl->m) { g_err = "row index out of range"; return CE_E_BADARG; }
    if (tpl->nnz_p > 0) {
        if (!tpl->p_indices || !tpl->p_indptr || tpl->p_indptr[tpl->n] != tpl->nnz_p) { g_err = "bad P structure"; return CE_E_BADARG; }
        for (int k = tpl->p_indptr[0]; k < tpl->nnz_p; k++) if (tpl->p_indices[k] < 0 || tpl->p_indices[k] >= tpl->n) { g_err = "P row index out of range"; return CE_E_BADARG; }
    }
    return CE_OK;
}

// what the engine derives from the template on the host and uploads as it stands
struct HostIndex {
    std::vector<int> colidx, rowcone, qoff, soff, sord;      // column of every structural entry; cone layout of the rows
    std::vector<int> rptr, rcol, rsrc, bpos;                 // CSR of the A part (entry positions refer to the boundary's value order) and the b entry of every row
    std::vector<int> drow, rowslot, srow_col, scol_ptr, scol_row, sing_i;      // split into rows with one entry / rows with several (filled when sp_RP > 0)
};
// sizes and cone layout: fills h.T (without its device pointers), h.q, h.psd_first and the host copy of the P structure
static void index_cones(const ce_template *tpl, ce_engine &h, HostIndex &X) {
    plan_sizes(tpl, h.T, X.qoff, X.soff);
    h.psd_first = X.soff[0];      // (= first row after the second-order cones: PSD blocks, then exponential / power triples, follow)
    X.colidx.resize(tpl->nnz_aug); X.rowcone.assign(tpl->m, -1);
    for (int j = 0; j <= tpl->n; j++)
        for (int k = tpl->indptr[j]; k < tpl->indptr[j + 1]; k++) X.colidx[k] = j;
    for (int c = 0; c < tpl->nq; c++) for (int i = 0; i < tpl->q[c]; i++) X.rowcone[X.qoff[c] + i] = c;
    X.sord.assign(std::max(tpl->ns, 1), 0);
    for (int c = 0; c < tpl->ns; c++) X.sord[c] = tpl->s[c];
    h.q.assign(tpl->q, tpl->q + tpl->nq);
    if (tpl->nnz_p > 0) {
        h.nnz_p = tpl->nnz_p; h.p_rows.resize(tpl->nnz_p); h.p_cols.resize(tpl->nnz_p);
        bool upper = true, lower = true;
        for (int j = 0; j < tpl->n; j++)
            for (int k = tpl->p_indptr[j]; k < tpl->p_indptr[j + 1]; k++) { const int i = tpl->p_indices[k]; h.p_rows[k] = i; h.p_cols[k] = j; upper = upper && i <= j; lower = lower && i >= j; }
        h.p_tri = (upper || lower) ? 1 : 0;
    }
}
// CSR of the A part + the singleton-row split, for the shared-A kernels; sets h.sp_r / h.sp_RP
static void index_csr_split(const ce_template *tpl, ce_engine &h, HostIndex &X) {
    const int n = tpl->n, m = tpl->m, nnzA = tpl->indptr[n];
    X.rptr.assign(m + 1, 0); X.rcol.resize(std::max(nnzA, 1)); X.rsrc.resize(std::max(nnzA, 1));
    for (int k = 0; k < nnzA; k++) X.rptr[tpl->indices[k] + 1]++;
    for (int i = 0; i < m; i++) X.rptr[i + 1] += X.rptr[i];
    std::vector<int> fill(X.rptr.begin(), X.rptr.end() - 1);
    for (int j = 0; j < n; j++)
        for (int k = tpl->indptr[j]; k < tpl->indptr[j + 1]; k++) { const int pos = fill[tpl->indices[k]]++; X.rcol[pos] = j; X.rsrc[pos] = k; }
    X.bpos.assign(m, -1);
    for (int k = tpl->indptr[n]; k < tpl->indptr[n + 1]; k++) X.bpos[tpl->indices[k]] = k;
    // split: rows with one entry / rows with several
    X.rowslot.assign(m, -1); X.srow_col.assign(m, -1);
    X.drow = dense_rows(tpl);
    for (int a = 0; a < (int)X.drow.size(); a++) X.rowslot[X.drow[a]] = a;
    for (int i = 0; i < m; i++) if (X.rptr[i + 1] - X.rptr[i] == 1) X.srow_col[i] = X.rcol[X.rptr[i]];
    h.sp_RP = split_RP((int)X.drow.size(), &h.sp_r);
    if (h.sp_RP == 0) return;
    X.scol_ptr.assign(n + 1, 0);
    for (int i = 0; i < m; i++) if (X.srow_col[i] >= 0) X.scol_ptr[X.srow_col[i] + 1]++;
    for (int j = 0; j < n; j++) X.scol_ptr[j + 1] += X.scol_ptr[j];
    X.scol_row.resize(std::max(X.scol_ptr[n], 1));
    std::vector<int> sfill(X.scol_ptr.begin(), X.scol_ptr.end() - 1);
    for (int i = 0; i < m; i++) if (X.srow_col[i] >= 0) X.scol_row[sfill[X.srow_col[i]]++] = i;
    if (X.drow.empty()) X.drow.push_back(0);
    X.sing_i.assign(n, -1);      // the one singleton row of a column (-1: none, -2: several)
    for (int j = 0; j < n; j++) { const int cnt = X.scol_ptr[j + 1] - X.scol_ptr[j]; X.sing_i[j] = cnt == 1 ? X.scol_row[X.scol_ptr[j]] : (cnt == 0 ? -1 : -2); }
}

// k_fwd2's gather maps for the planned variant: thread-major, rows padded to 16 bytes (ce_forward_v2.h idx_stride); -1 = structural zero
struct GatherMaps { std::vector<int> iat, iar, ib, ip, pmap, row_perm, k_rowcone, k_qoff; };
static void build_gather_maps(const ce_template *tpl, const ce_engine &h, GatherMaps &G) {
    const DevT &T = h.T; const F2Geom &g = F2_ROWS[h.plan.f2_variant].g;
    const int S1 = (g.T1 + 3) & ~3, S2 = (g.T2 + 3) & ~3, SG = (g.TG + 3) & ~3;
    std::vector<int> pos((size_t)T.m * T.n, -1), ib0(T.m, -1), korig(T.m);
    for (int j = 0; j <= T.n; j++)
        for (int k = tpl->indptr[j]; k < tpl->indptr[j + 1]; k++) { if (j < T.n) pos[(size_t)tpl->indices[k] * T.n + j] = k; else ib0[tpl->indices[k]] = k; }
    if (h.plan.wl) { pack_rows(tpl, 64 / g.CHA, korig, G.k_rowcone, G.k_qoff); G.row_perm = korig; }
    else for (int i = 0; i < T.m; i++) korig[i] = i;
    G.ib.assign(T.m, -1); G.iat.assign((size_t)S1 * g.NTH, -1); G.iar.assign((size_t)S2 * g.NTH, -1);
    for (int r = 0; r < T.m; r++) G.ib[r] = ib0[korig[r]];
    for (int t = 0; t < g.NTH; t++) {
        const int j1 = t / g.CHT, c1 = t % g.CHT, i2 = t / g.CHA, c2 = t % g.CHA;
        for (int k = 0; k < g.T1; k++) { const int r = g.T1 * c1 + k; if (j1 < T.n && r < T.m) G.iat[(size_t)t * S1 + k] = pos[(size_t)korig[r] * T.n + j1]; }
        for (int k = 0; k < g.T2; k++) { const int c = g.T2 * c2 + k; if (i2 < T.m && c < T.n) G.iar[(size_t)t * S2 + k] = pos[(size_t)korig[i2] * T.n + c]; }
    }
    if (!h.plan.qp_native) return;
    // quadratic objective: gather map of the (jg, cg) tile layout and the dense n x n entry map
    G.pmap.assign((size_t)T.n * T.n, -1); G.ip.assign((size_t)SG * g.NTH, -1);
    for (int k = 0; k < h.nnz_p; k++) { G.pmap[(size_t)h.p_rows[k] * T.n + h.p_cols[k]] = k; if (h.p_tri) G.pmap[(size_t)h.p_cols[k] * T.n + h.p_rows[k]] = k; }
    for (int t = 0; t < g.NTH; t++) {
        const int jg = t / g.CHG, cg = t % g.CHG;
        for (int k = 0; k < g.TG; k++) { const int c = g.TG * cg + k; if (jg < T.n && c < T.n) G.ip[(size_t)t * SG + k] = G.pmap[(size_t)jg * T.n + c]; }
    }
}

static constexpr size_t VALUE_LDS_MAX = LDS_LIMIT - 1024;      // dynamic LDS of the kernels of ce_value.h (they also hold a few static bytes: the workgroup votes)
static int upload_engine(const ce_template *tpl, ce_engine &h, const HostIndex &X, const GatherMaps &G) {
    DevT &T = h.T;
    HIPCHK(h.d_pw.upload(tpl->p, tpl->np));
    HIPCHK(h.d_rowidx.upload(tpl->indices, tpl->nnz_aug)); HIPCHK(h.d_colidx.upload(X.colidx)); HIPCHK(h.d_rowcone.upload(X.rowcone)); HIPCHK(h.d_qoff.upload(X.qoff));
    HIPCHK(h.d_soff.upload(X.soff)); HIPCHK(h.d_sord.upload(X.sord));
    T.pw = h.d_pw.get(); T.rowidx = h.d_rowidx.get(); T.colidx = h.d_colidx.get(); T.rowcone = h.d_rowcone.get(); T.qoff = h.d_qoff.get(); T.soff = h.d_soff.get(); T.sord = h.d_sord.get();
    HIPCHK(h.d_csc_ptr.upload(tpl->indptr, tpl->n + 1)); HIPCHK(h.d_csr_ptr.upload(X.rptr)); HIPCHK(h.d_csr_col.upload(X.rcol)); HIPCHK(h.d_csr_src.upload(X.rsrc)); HIPCHK(h.d_bpos.upload(X.bpos));
    if (h.sp_RP > 0) {
        HIPCHK(h.d_sp_drow.upload(X.drow)); HIPCHK(h.d_sp_srow_col.upload(X.srow_col)); HIPCHK(h.d_sp_scol_ptr.upload(X.scol_ptr)); HIPCHK(h.d_sp_scol_row.upload(X.scol_row));
        HIPCHK(h.d_sp_rowslot.upload(X.rowslot)); HIPCHK(h.d_sp_sing_i.upload(X.sing_i));
        HIPCHK(h.d_sp_sing_v.reserve(T.n)); HIPCHK(h.d_sp_AdT.reserve((size_t)T.n * h.sp_RP)); HIPCHK(h.d_sp_sval.reserve(T.m));
    }
    HIPCHK(h.d_idx_at.upload(G.iat)); HIPCHK(h.d_idx_ar.upload(G.iar)); HIPCHK(h.d_idx_b.upload(G.ib));      // (empty unless k_fwd2 is planned)
    HIPCHK(h.d_row_perm.upload(G.row_perm)); HIPCHK(h.d_k_rowcone.upload(G.k_rowcone)); HIPCHK(h.d_k_qoff.upload(G.k_qoff));
    if (h.plan.wl) h.wl_nq = (int)G.k_qoff.size() - 1;
    if (h.plan.qp_native) { HIPCHK(h.d_idx_p.upload(G.ip)); HIPCHK(h.d_pmap.upload(G.pmap)); HIPCHK(h.d_prow.upload(h.p_rows)); HIPCHK(h.d_pcol.upload(h.p_cols)); }
    HIPCHK(ce_setattr_fwd_generic((int)LDS_LIMIT)); HIPCHK(ce_setattr_fwd_rt((int)LDS_LIMIT));
    HIPCHK(ce_setattr_fwd2_plain((int)LDS_LIMIT)); HIPCHK(ce_setattr_fwd2_psd((int)LDS_LIMIT)); HIPCHK(ce_setattr_fwd2_qp((int)LDS_LIMIT));
    HIPCHK(ce_setattr_bwd_rt_plain((int)LDS_LIMIT)); HIPCHK(ce_setattr_bwd_rt_psd((int)LDS_LIMIT)); HIPCHK(ce_setattr_bwd_generic((int)LDS_LIMIT)); HIPCHK(ce_setattr_ns((int)LDS_LIMIT)); HIPCHK(ce_setattr_ns_qp((int)LDS_LIMIT)); HIPCHK(ce_setattr_ns_tri((int)LDS_LIMIT)); HIPCHK(ce_setattr_ns_many((int)LDS_LIMIT)); HIPCHK(ce_setattr_ns_jvp_many((int)LDS_LIMIT)); HIPCHK(ce_setattr_ns_jvp_qp_many((int)LDS_LIMIT)); HIPCHK(ce_setattr_ns_vjp_qp_many((int)LDS_LIMIT)); HIPCHK(ce_setattr_ns_vjp_tri_many((int)LDS_LIMIT)); HIPCHK(ce_setattr_ns_jvp_tri_many((int)LDS_LIMIT)); HIPCHK(ce_setattr_ns_psd((int)LDS_LIMIT)); HIPCHK(ce_setattr_ns_vjp_psd_many((int)LDS_LIMIT)); HIPCHK(ce_setattr_ns_jvp_psd_many((int)LDS_LIMIT)); HIPCHK(ce_setattr_ns_psd_tri((int)LDS_LIMIT)); HIPCHK(ce_setattr_ns_vjp_psd_tri_many((int)LDS_LIMIT)); HIPCHK(ce_setattr_ns_jvp_psd_tri_many((int)LDS_LIMIT));
    HIPCHK(ce_setattr_value((int)VALUE_LDS_MAX)); HIPCHK(ce_setattr_lpgd((int)VALUE_LDS_MAX)); HIPCHK(ce_setattr_check((int)VALUE_LDS_MAX));
    HIPCHK(hipFuncSetAttribute((const void *)k_expand_dA, hipFuncAttributeMaxDynamicSharedMemorySize, (int)EXPAND_LDS_MAX));
    HIPCHK(ce_setattr_param_grad((int)LDS_LIMIT));
    return CE_OK;
}

extern "C" {

const char *ce_last_error(void) { return g_err.c_str(); }
int ce_abi_version(void) { return CE_ABI_VERSION; }
int ce_set_lsqr_variant(ce_handle h, int variant) {
    if (!h || variant < 0 || variant > 1) { g_err = "ce_set_lsqr_variant: variant must be 0 (LSQR) or 1 (LSMR)"; return CE_E_BADARG; }
    h->lsqr_variant = variant;
    return CE_OK;
}
// Anderson acceleration: k_fwd2 when its history fits LDS; the first-generation register-tiled k_forward_rt and the size-generic k_forward keep the history in global memory.
int ce_acceleration_available(ce_handle h) { return (h && ((h->plan.fwd_mode == FWD_V2 && h->plan.aa_ok) || h->plan.fwd_mode != FWD_V2)) ? 1 : 0; }
int ce_struct_size(int which) { return which == 0 ? (int)sizeof(ce_template) : which == 1 ? (int)sizeof(ce_settings) : -1; }

void ce_default_settings(ce_settings *s) {
    s->eps_abs = 1e-4; s->eps_rel = 1e-4; s->eps_infeas = 1e-7; s->alpha = 1.5; s->rho_x = 1e-6; s->scale = 0.1;
    s->max_iters = 100000; s->normalize = 1; s->adaptive_scale = 1; s->warm_start = 0; s->acceleration_lookback = 10; s->acceleration_interval = 10;   // SCS 3 defaults, which diffcp forwards (diffcp_if.py:356-367)
}

int ce_create(const ce_template *tpl, int device, ce_handle *out) {
    int rc = validate_template(tpl, out);
    if (rc) return rc;
    HIPCHK(hipSetDevice(device));
    std::unique_ptr<ce_engine> h(new ce_engine());      // (a failed create frees whatever it allocated)
    h->device = device;
    HostIndex X;
    index_cones(tpl, *h, X);
    index_csr_split(tpl, *h, X);
    rc = plan_engine(tpl, h->T, h->nnz_p, read_plan_env(), h->plan);
    if (rc) return rc;
    h->wave_variant = fwd_wave_variant(tpl->n, tpl->m, tpl->z, tpl->l, tpl->nq, tpl->q, tpl->ns, tpl->nep, tpl->np, tpl->nnz_p);
    h->wave_lds = h->wave_variant >= 0 ? fwd_wave_lds_bytes(h->wave_variant, tpl->n, tpl->m) : 0;
    h->T.f2_neumann = h->plan.f2_neumann; h->T.gen_blocked_f = h->plan.gen_blocked_f; h->T.gen_blocked_b = h->plan.gen_blocked_b;
    GatherMaps G;
    if (h->plan.fwd_mode == FWD_V2) build_gather_maps(tpl, *h, G);
    rc = upload_engine(tpl, *h, X, G);
    if (rc) return rc;
    *out = h.release();
    return CE_OK;
}

int ce_adjoint_ns_variant(ce_handle h) { return h ? h->plan.ns_variant : -1; }
int ce_qp_ns_variant(ce_handle h) { return h ? h->plan.qp_ns_variant : -1; }
int ce_tri_ns_variant(ce_handle h) { return h ? h->plan.tri_ns_variant : -1; }
int ce_psd_ns_variant(ce_handle h) { return h ? h->plan.psd_ns_variant : -1; }
long ce_psd_ns_lds(ce_handle h) { return (h && h->plan.psd_ns_variant >= 0) ? (long)h->plan.psd_ns_lds : 0; }
// the many-cotangent mode rebuilds every cotangent's vectors in the buffers of the plain adjoint: its row and footprint are ns_variant's, and like the kernel
// behind ce_vjp it only runs in front of the LSQR re-solve
int ce_vjp_many_variant(ce_handle h) { return (h && h->plan.ns_variant >= 0 && resolve_lds_fits(h->T, h->psd_first)) ? h->plan.ns_variant : -1; }
// the parameter gradient from the factors runs behind that mode (ce_vjp_many_params) and behind the single-cotangent adjoint's factor mode (ce_vjp_params): the same
// templates -- k_param_grad's smallest tile holds two pairs' factors, 16 (3 n + 2 m + 2) bytes, wherever the elimination's own footprint fits -- and the packed
// (i, j) of a map entry asks for m < 2^16, n < 2^15, which n <= 108 and an A that fits LDS imply
int ce_param_grad_variant(ce_handle h) { return (ce_vjp_many_variant(h) >= 0 && h->T.m < (1 << 16)) ? h->plan.ns_variant : -1; }
// the many-tangent modes rebuild every tangent's vectors in the buffers of ce_jvp / ce_jvp_qp: their rows and footprints.  Plain kind: the rule of ce_jvp without the
// triples (TRI keeps K launches: ce_backward_ns.h).  Either kind is kept in-kernel only while its K = 8 bracket lies below K single-tangent calls
// (profiles/jvp_many/): a kind that fails that is switched off here, and ConeEngine.jvp_many runs its loop.
int ce_jvp_many_variant(ce_handle h) { return (h && !h->plan.qp_native && h->plan.ns_variant >= 0 && resolve_lds_fits(h->T, h->psd_first)) ? h->plan.ns_variant : -1; }
int ce_jvp_qp_many_variant(ce_handle h) { return (h && h->plan.qp_native && h->plan.qp_ns_variant >= 0) ? h->plan.qp_ns_variant : -1; }
int ce_vjp_qp_many_variant(ce_handle h) { return (h && h->plan.qp_native && h->plan.qp_ns_variant >= 0) ? h->plan.qp_ns_variant : -1; }
// the many-cotangent mode with exponential / power triples runs on the footprint of the triples' forward modes: tri_ns_variant's row (the tri planner already asks
// that the LSQR vectors of the re-solve fit LDS)
int ce_vjp_tri_many_variant(ce_handle h) { return (h && h->plan.tri_ns_variant >= 0) ? h->plan.tri_ns_variant : -1; }
// the many-tangent mode with triples: the same rule and row (its rebuild lives in the buffers the single-tangent mode and the many-cotangent mode use on tri_ns_lds:
// no shape is excluded by the footprint)
int ce_jvp_tri_many_variant(ce_handle h) { return (h && h->plan.tri_ns_variant >= 0) ? h->plan.tri_ns_variant : -1; }
// the many-cotangent and many-tangent modes with PSD blocks run on the footprint of the blocks' forward modes: psd_ns_variant's row (the psd planner already asks
// that the LSQR vectors of the re-solve fit LDS; the rotation of a right-hand side lives in the (X, W) pairs the single-tangent mode rotates A on)
int ce_vjp_psd_many_variant(ce_handle h) { return (h && h->plan.psd_ns_variant >= 0) ? h->plan.psd_ns_variant : -1; }
int ce_jvp_psd_many_variant(ce_handle h) { return (h && h->plan.psd_ns_variant >= 0) ? h->plan.psd_ns_variant : -1; }
// a template with PSD blocks AND triples: one row and footprint (both kinds' segments) for its four modes; the planner already asks that the LSQR vectors of the
// re-solve fit LDS
int ce_psd_tri_ns_variant(ce_handle h) { return h ? h->plan.psd_tri_ns_variant : -1; }
long ce_psd_tri_ns_lds(ce_handle h) { return (h && h->plan.psd_tri_ns_variant >= 0) ? (long)h->plan.psd_tri_ns_lds : 0; }
int ce_vjp_psd_tri_many_variant(ce_handle h) { return (h && h->plan.psd_tri_ns_variant >= 0) ? h->plan.psd_tri_ns_variant : -1; }
int ce_jvp_psd_tri_many_variant(ce_handle h) { return (h && h->plan.psd_tri_ns_variant >= 0) ? h->plan.psd_tri_ns_variant : -1; }
int ce_set_adjoint_resolve(ce_handle h, int enable, double atol, double btol, double conlim, int iter_lim) {
    if (!h) { g_err = "null argument"; return CE_E_BADARG; }
    h->resolve = enable != 0;
    h->rs_atol = atol > 0 ? atol : 1e-8; h->rs_btol = btol > 0 ? btol : 1e-8; h->rs_conlim = conlim; h->rs_iter_lim = iter_lim > 0 ? iter_lim : 0;
    return CE_OK;
}
int ce_destroy(ce_handle h) {
    if (!h) return CE_OK;
    hipSetDevice(h->device);
    if (h->d_psd_stats.get()) {
        unsigned long long c[16] = {0};
        if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(c, h->d_psd_stats.get(), sizeof(c), hipMemcpyDeviceToHost) == hipSuccess)
            fprintf(stderr, "[cone_engine] PSD projections %llu: refinement steps %llu (%.2f per projection), warm Jacobi fall-backs %llu, cold starts %llu; "
                            "clock64 ticks per projection %.0f (of which Jacobi sweeps %.0f), per iteration up to the end of the projection %.0f\n",
                    c[0], c[1], c[0] ? (double)c[1] / (double)c[0] : 0.0, c[2], c[3], c[0] ? (double)c[4] / c[0] : 0.0, c[0] ? (double)c[6] / c[0] : 0.0, c[0] ? (double)c[5] / c[0] : 0.0),
            fprintf(stderr, "[cone_engine]   ticks per projection by phase: T=SV,R %.0f | D=V'T %.0f | E %.0f | reduce %.0f | V+=VE %.0f | X, store %.0f\n",
                    (double)c[8] / (c[0] ? c[0] : 1), (double)c[9] / (c[0] ? c[0] : 1), (double)c[10] / (c[0] ? c[0] : 1), (double)c[11] / (c[0] ? c[0] : 1), (double)c[12] / (c[0] ? c[0] : 1), (double)c[13] / (c[0] ? c[0] : 1));
    }
    delete h;
    return CE_OK;
}

// (rows x cols) row-major -> (cols x rows) row-major
static void launch_transpose(hipStream_t st, const double *in, double *out, int rows, int cols) {
    static const int ts = [] { const char *e = getenv("CE_TR_TILE"); return (e && atoi(e) == 32) ? 32 : 64; }();
    if (ts == 32) hipLaunchKernelGGL(k_transpose<32>, dim3((cols + 31) / 32, (rows + 31) / 32), dim3(256), 0, st, in, out, rows, cols);
    else hipLaunchKernelGGL(k_transpose<64>, dim3((cols + 63) / 64, (rows + 63) / 64), dim3(256), 0, st, in, out, rows, cols);
}
// k_expand_dA's launch shape for a batch: slabs of the value order so that tiles x slabs is about four workgroups per CU (two are resident on one: a tile's
// x, y and v take 8 (n + 2 m) 33 bytes, 66 KB at the metric shape), no slab shorter than 256 entries.  false: the template is not the kernel's (a tile beyond
// EXPAND_LDS_MAX, indices beyond the packed (i, j) pair, a row too short for the m factors) -- the caller keeps the layout pass.
struct ExpandPlan { int slab, slabs; size_t lds; };
static bool expand_dA_plan(const DevT &T, int B, ExpandPlan *ex) {
    const int K = T.nnz_aug;
    if (T.m >= (1 << 16) || T.n >= (1 << 15) || K < T.m) return false;
    const int tiles = (B + EXP_TB - 1) / EXP_TB;
    int slabs = std::max(1, std::min((K + 255) / 256, (1024 + tiles - 1) / tiles));
    ex->slab = (K + slabs - 1) / slabs;
    ex->slabs = (K + ex->slab - 1) / ex->slab;
    ex->lds = expand_dA_lds_bytes(T.n, T.m, ex->slab);
    return ex->lds <= EXPAND_LDS_MAX;
}
struct ProfScope {
    ce_engine *h; int which; hipStream_t st; hipEvent_t a{}, b{}; bool on;
    ProfScope(ce_engine *h_, int w, hipStream_t s) : h(h_), which(w), st(s), on(((h_->prof >> w) & 1) != 0) {
        // events come from a pool filled by earlier scopes (ce_reset_profile returns them): creating a pair per launch cost host time in front of every
        // kernel of a profiled run -- bench.py's timed region is one
        if (on) {
            if (h->ev_pool.size() >= 2) { a = h->ev_pool.back(); h->ev_pool.pop_back(); b = h->ev_pool.back(); h->ev_pool.pop_back(); }
            else { hipEventCreate(&a); hipEventCreate(&b); }
            hipEventRecord(a, st);
        }
    }
    ~ProfScope() { if (on) { hipEventRecord(b, st); h->ev[which].push_back({a, b}); } }
};

// batch-minor (K x B) -> batch-major (B x K) when needed; returns the batch-major pointer
static int to_batch_major(ce_engine *h, int B, const double *vals, long sk, long sb, hipStream_t st, const double **out) {
    const int K = h->T.nnz_aug;
    if (sk == 1 && sb == K) { *out = vals; return CE_OK; }
    if (!(sb == 1 && sk == B)) { g_err = "A_vals must be contiguous batch-minor (sk=B,sb=1) or batch-major (sk=1,sb=nnz_aug)"; return CE_E_BADARG; }
    HIPCHK(h->wsA.reserve((size_t)B * K));
    {
        ProfScope ps(h, 2, st);
        launch_transpose(st, vals, h->wsA.get(), K, B);
    }
    *out = h->wsA.get();
    return CE_OK;
}

static int flush_dispatch_order(ce_engine *h, hipStream_t st, const int *sum_status, int *sum_out);      // (defined next to ce_set_dispatch_history)

int ce_qp_native(ce_handle h) { return (h && h->plan.qp_native) ? 1 : 0; }

int ce_solve(ce_handle h, int B, const double *A_vals, long sA_k, long sA_b, const double *q_vals, long sq_k, long sq_b,
             const ce_settings *settings, double *x, double *y, double *s, int *iters, int *status, double *resid, void *stream) {
    return ce_solve_qp(h, B, A_vals, sA_k, sA_b, q_vals, sq_k, sq_b, nullptr, settings, x, y, s, iters, status, resid, stream);
}

int ce_solve_qp(ce_handle h, int B, const double *A_vals, long sA_k, long sA_b, const double *q_vals, long sq_k, long sq_b,
                const double *P_vals, const ce_settings *settings, double *x, double *y, double *s, int *iters, int *status, double *resid, void *stream) {
    if (!h || B <= 0 || !A_vals || !q_vals || !x || !y || !s || !iters || !status) { g_err = "null argument"; return CE_E_BADARG; }
    const CePlan &P = h->plan;
    if (P_vals && !P.qp_native) { g_err = "quadratic objective: this template does not run P inside the kernels (ce_qp_native == 0); use the epigraph form"; return CE_E_UNSUPPORTED; }
    if (!P_vals && P.qp_native) { g_err = "template created with a P structure: P_vals is required"; return CE_E_BADARG; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    // (PSD / exponential / power cones beyond k_fwd2's sizes run on the size-generic kernel: FWD_GEN_*)
    if ((h->T.ns > 0 || h->T.nep + h->T.np > 0) && P.fwd_mode == FWD_RT) { g_err = "PSD / exponential / power cones: internal error, k_forward_rt selected"; return CE_E_UNSUPPORTED; }
    ce_settings S; if (settings) S = *settings; else ce_default_settings(&S);
    if (!ce_acceleration_available(h)) S.acceleration_lookback = 0;          // k_fwd2 (when its vectors fit LDS) and the size-generic kernel implement it
    if (S.acceleration_interval <= 0) S.acceleration_interval = 10;
    const double *Abm = nullptr;
    const bool transient = h->transient_solve;          // a solve issued from a backward pass (LPGD): no trace on the handle
    if (transient && !(sA_k == 1 && sA_b == h->T.nnz_aug)) { g_err = "transient solve: A_vals must be batch-major (the layout workspace may hold the retained forward inputs)"; return CE_E_BADARG; }
    int rc = to_batch_major(h, B, A_vals, sA_k, sA_b, st, &Abm);
    if (rc) return rc;
    if (!transient) { h->retained_A = Abm; h->retained_B = B; }
    const DevT &T = h->T;
    double *gA = nullptr, *gG = nullptr;
    if (P.fwd_mode == FWD_GEN_G_GLOBAL || P.fwd_mode == FWD_GEN_GLOBAL) {
        size_t perA = (P.fwd_mode == FWD_GEN_GLOBAL) ? (size_t)T.m * T.lda : 0, perG = (size_t)T.n * T.ldg;
        HIPCHK(h->gws.reserve((size_t)B * (perA + perG)));
        gG = h->gws.get(); gA = h->gws.get() + (size_t)B * perG;
    }
    double *aa_ws = nullptr;
    if (P.fwd_mode != FWD_V2 && S.acceleration_lookback > 0) {      // k_forward_rt and the size-generic kernel keep the acceleration history in global memory ([B][4][lp], shared with the shared-A kernel's)
        const size_t l = (size_t)T.n + T.m + 1, lp = l + (l & 1);
        HIPCHK(h->d_aa_ws.reserve((size_t)B * 4 * lp));
        aa_ws = h->d_aa_ws.get();
    }
    bool fa_iters2 = false;
    {
        ProfScope ps(h, 0, st);
        CeFwdArgs fa{};
        fa.aa_ws = aa_ws;
        fa.T = T; fa.S = S; fa.Abm = Abm; fa.q = q_vals; fa.sqk = sq_k; fa.sqb = sq_b; fa.idx_at = h->d_idx_at.get(); fa.idx_ar = h->d_idx_ar.get(); fa.idx_b = h->d_idx_b.get();
        fa.x = x; fa.y = y; fa.s = s; fa.iters = iters; fa.status = status; fa.resid = resid; fa.P = P_vals; fa.nnz_p = h->nnz_p; fa.idx_p = h->d_idx_p.get(); fa.gA = gA; fa.gG = gG;
        int lrc;
        if (h->dispatch_history && !transient && P.fwd_mode == FWD_V2) {
            rc = flush_dispatch_order(h, st, nullptr, nullptr); if (rc) return rc;          // (a solve whose status was never summarised: the order is still owed)
            HIPCHK(h->d_iters2.reserve(B));
            fa.iters2 = h->d_iters2.get(); fa_iters2 = true;
        }
        fa.order = (h->dispatch_history && !transient && h->order_B == B && P.fwd_mode == FWD_V2) ? h->d_order.get() : nullptr;
        if (P.fwd_mode == FWD_V2) {
            fa.T.ldg = P.f2_ldg;
            if (P.wl) {      // rows packed for the wave-local cone exchange: the kernel sees the cone layout in ITS row order
                fa.row_perm = h->d_row_perm.get(); fa.T.rowcone = h->d_k_rowcone.get(); fa.T.qoff = h->d_k_qoff.get(); fa.T.nq = h->wl_nq; fa.T.l = 0;
            }
            if (P_vals) lrc = ce_launch_fwd2_qp(P.f2_variant, B, P.fwd_lds, st, fa);
            else if (T.ns > 0 || T.nep + T.np > 0) lrc = ce_launch_fwd2_psd(P.f2_variant, B, P.fwd_lds, st, fa);
            else lrc = ce_launch_fwd2_plain(P.f2_variant, B, P.fwd_lds, st, fa);
        } else if (P.fwd_mode == FWD_RT) {
            fa.T.lda = P.rt_lda;
            lrc = ce_launch_fwd_rt(P.rt_variant, B, P.fwd_lds, st, fa);
        } else lrc = ce_launch_fwd_generic(P.fwd_mode, B, P.fwd_lds, st, fa);
        if (lrc) { g_err = "internal: no forward kernel for the planned variant"; return CE_E_BADARG; }
    }
    HIPCHK(hipGetLastError());
    if (fa_iters2) { h->order_pending_B = B; h->last_status = status; }          // (computed by flush_dispatch_order, off the critical path)
    return CE_OK;
}

// k_fwd_wave: one instance per wave, for the small templates fwd_wave_variant serves (ce_lds_fwd_wave.h).  The arguments, layouts and retention of ce_solve; the
// dispatch history is left alone (the kernel takes the instances in index order)
int ce_wave_variant(ce_handle h) { return h ? h->wave_variant : -1; }
int ce_wave_lds(ce_handle h) { return (h && h->wave_variant >= 0) ? (int)h->wave_lds : 0; }
int ce_wave_occupancy(ce_handle h) {
    if (!h || h->wave_variant < 0) return 0;
    int blocks = 0;
    if (hipSetDevice(h->device) != hipSuccess || ce_occupancy_fwd_wave(h->wave_variant, h->wave_lds, &blocks) != hipSuccess) return 0;
    return blocks;
}
int ce_solve_wave(ce_handle h, int B, const double *A_vals, long sA_k, long sA_b, const double *q_vals, long sq_k, long sq_b,
                  const ce_settings *settings, double *x, double *y, double *s, int *iters, int *status, double *resid, void *stream) {
    if (!h || B <= 0 || !A_vals || !q_vals || !x || !y || !s || !iters || !status) { g_err = "null argument"; return CE_E_BADARG; }
    if (h->wave_variant < 0) {
        g_err = std::string("ce_solve_wave: ") + fwd_wave_refusal(h->T.n, h->T.m, h->T.ns, h->T.nep, h->T.np, h->nnz_p) + "; use ce_solve";
        return CE_E_UNSUPPORTED;
    }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    ce_settings S; if (settings) S = *settings; else ce_default_settings(&S);
    if (S.acceleration_interval <= 0) S.acceleration_interval = 10;
    const double *Abm = nullptr;
    const bool transient = h->transient_solve;
    if (transient && !(sA_k == 1 && sA_b == h->T.nnz_aug)) { g_err = "transient solve: A_vals must be batch-major (the layout workspace may hold the retained forward inputs)"; return CE_E_BADARG; }
    int rc = to_batch_major(h, B, A_vals, sA_k, sA_b, st, &Abm);
    if (rc) return rc;
    if (!transient) { h->retained_A = Abm; h->retained_B = B; }
    {
        ProfScope ps(h, 0, st);
        CeFwdArgs fa{};
        fa.T = h->T; fa.S = S; fa.Abm = Abm; fa.q = q_vals; fa.sqk = sq_k; fa.sqb = sq_b;
        fa.x = x; fa.y = y; fa.s = s; fa.iters = iters; fa.status = status; fa.resid = resid;
        if (ce_launch_fwd_wave(h->wave_variant, B, h->wave_lds, st, fa)) { g_err = "internal: no wave kernel for the selected row"; return CE_E_BADARG; }
    }
    HIPCHK(hipGetLastError());
    return CE_OK;
}

int ce_vjp(ce_handle h, int B, const double *A_vals, long sA_k, long sA_b, const double *q_vals, long sq_k, long sq_b,
           const double *x, const double *y, const double *s, const double *dx, const double *dy,
           double *dA_vals, long sdA_k, long sdA_b, double *dq_vals, long sdq_k, long sdq_b, int *adj_status, void *stream) {
    // b, c do not enter the elimination (r_tau pinned to 0); they do enter diffcp's full system, which the instances the elimination flags as rank deficient
    // are re-solved on (ce_set_adjoint_resolve): q_vals == NULL switches the re-solve off for this call
    if (!h) { g_err = "null argument"; return CE_E_BADARG; }
    h->call_q = q_vals; h->call_sqk = sq_k; h->call_sqb = sq_b;
    const int rc = ce_vjp_qp(h, B, A_vals, sA_k, sA_b, nullptr, x, y, s, dx, dy, dA_vals, sdA_k, sdA_b, dq_vals, sdq_k, sdq_b, nullptr, adj_status, stream);
    h->call_q = nullptr;
    return rc;
}

static int vjp_lsqr_launch(ce_handle h, int B, const double *A_vals0, long sA_b, int per_inst, const double *q_vals, long sq_k, long sq_b,
                           const double *x, const double *y, const double *s, const double *dx, const double *dy,
                           double *dA_bm, double *dq_vals, long sdq_k, long sdq_b, int *adj_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream,
                           const int *sel = nullptr, int status_or = 0, int *sel_reset = nullptr, const SaJvp *fwd = nullptr, const SaWalkMany *many = nullptr);
// The re-solve list of ce_vjp_qp and ce_jvp.  The elimination kernel of a call appends the instances whose system it found rank deficient (or too large for its
// tile) to a device-side list; a fixed grid of LSQR workgroups behind it walks the list and overwrites those instances' results with diffcp's minimum-norm answer
// (k_sa_lsqr with the instance's own A).  No host round trip; an empty list costs one launch of workgroups that return at once.
// TWO lists (count | entries) in d_fix, used alternately: the LSQR launch of a call empties the list of the call before -- no memset per call.
struct FixLists { int *cur, *oth; };
static bool resolve_fits(const ce_engine *h) {      // the LSQR vectors of one instance (CSR / CSC products: per-instance values) fit LDS
    return resolve_lds_fits(h->T, h->psd_first);          // (ce_plan.h: the plan of the triples' elimination asks the same question)
}
// part one, in front of the elimination launch: the list this call appends to and the other one; d_fix grows and is zeroed on first use for a batch size
static int resolve_lists(ce_handle h, int B, hipStream_t st, FixLists *L) {
    if (h->fix_cap < B) {
        HIPCHK(h->d_fix.reserve(2 * ((size_t)B + 1))); h->fix_cap = B; h->fix_par = 0;
        HIPCHK(hipMemsetAsync(h->d_fix.get(), 0, sizeof(int) * 2 * ((size_t)B + 1), st));
    }
    L->cur = h->d_fix.get() + (size_t)h->fix_par * (h->fix_cap + 1); L->oth = h->d_fix.get() + (size_t)(1 - h->fix_par) * (h->fix_cap + 1);
    return CE_OK;
}
// part two, behind it: lsqr(grid, sel, status_or, sel_reset) launches the LSQR kernel over the current list; the served instances get 4 | 8 ("rank deficient,
// re-solved by LSQR") OR-ed into their status.  The caller's ProfScope brackets the launch already: the engine's profiling is off for its duration.
extern "C++" {
template <class F>
static int resolve_run(ce_handle h, int B, const FixLists &L, F &&lsqr) {
    const int grid = B < 768 ? B : 768;          // three workgroups per CU: what the LSQR kernel's LDS allows
    const int prof_keep = h->prof; h->prof = 0;
    const int rc = lsqr(grid, L.cur, 4 | 8, L.oth);
    h->fix_par ^= 1;
    h->prof = prof_keep;
    return rc;
}
}  // extern "C++"
int ce_vjp_qp(ce_handle h, int B, const double *A_vals, long sA_k, long sA_b, const double *P_vals,
              const double *x, const double *y, const double *s, const double *dx, const double *dy,
              double *dA_vals, long sdA_k, long sdA_b, double *dq_vals, long sdq_k, long sdq_b, double *dP_vals, int *adj_status, void *stream) {
    const CeParamGradArgs *const pg = h ? h->pg : nullptr;          // (ce_vjp_params: no dA_vals; the workspace row of an instance holds its factors, or its re-solved row)
    if (!h || B <= 0 || !x || !y || !s || !dx || !dy || (!dA_vals && !pg) || !dq_vals) { g_err = "null argument"; return CE_E_BADARG; }
    const CePlan &P = h->plan;
    if ((P_vals != nullptr) != P.qp_native || (P_vals && !dP_vals)) { g_err = "quadratic objective: P_vals / dP_vals must be given exactly when ce_qp_native(h) == 1"; return CE_E_BADARG; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const DevT &T = h->T;
    if ((T.ns > 0 || T.nep + T.np > 0) && P.bwd_mode == BWD_RT && !BRT_HAS_PSD) { g_err = "PSD / exponential cones: the register-tiled adjoint was built without them"; return CE_E_UNSUPPORTED; }
    const double *Abm = nullptr;
    int rc;
    if (A_vals) { rc = to_batch_major(h, B, A_vals, sA_k, sA_b, st, &Abm); if (rc) return rc; }
    else { if (!h->retained_A || h->retained_B != B) { g_err = "no retained forward inputs"; return CE_E_STATE; } Abm = h->retained_A; }
    const int K = T.nnz_aug;
    double *dAbm = nullptr; bool need_tr = false;
    if (pg) { HIPCHK(h->wsdA.reserve((size_t)B * K)); dAbm = h->wsdA.get(); }
    else if (sdA_k == 1 && sdA_b == K) dAbm = dA_vals;
    else if (sdA_b == 1 && sdA_k == B) { HIPCHK(h->wsdA.reserve((size_t)B * K)); dAbm = h->wsdA.get(); need_tr = true; }
    else { g_err = "dA_vals must be contiguous batch-minor or batch-major"; return CE_E_BADARG; }
    double *gA = nullptr, *gK = nullptr;
    if (P.bwd_mode == BWD_GEN_K_GLOBAL || P.bwd_mode == BWD_GEN_GLOBAL) {
        size_t perA = (P.bwd_mode == BWD_GEN_GLOBAL) ? (size_t)T.m * T.lda : 0, perK = (size_t)P.nkcap * P.ldk;
        HIPCHK(h->gws.reserve((size_t)B * (perA + perK)));
        gK = h->gws.get(); gA = h->gws.get() + (size_t)B * perK;
    }
    // Rank-deficient adjoint systems (redundant equality rows, degenerate active sets): the elimination kernels set the free variables to zero -- a BASIC
    // solution -- where the reference's LSQR (diffcp_if.py:86 -> adj_batch) returns the minimum-norm one: those instances go through the re-solve list above.
    const bool do_fix = h->resolve && h->call_q && !P_vals && resolve_fits(h);
    FixLists fix{nullptr, nullptr};
    if (do_fix) { rc = resolve_lists(h, B, st, &fix); if (rc) return rc; }
    // Factor mode: a batch-minor dA behind the search-free adjoint is written once, by k_expand_dA from (x, y, -dq, r_y), instead of batch-major by the adjoint and
    // again by the layout pass; the adjoint stores r_y at the head of the instance's row of wsdA, where a re-solved instance's whole row lands as before.  The
    // expansion tells the two apart by bit 8 of adj_status, so a call without one keeps the layout pass (as does a template whose tile exceeds the kernel's LDS).
    ExpandPlan ex{};
    const bool factors = pg ? true : (need_tr && do_fix && P.ns_variant >= 0 && adj_status && expand_dA_plan(T, B, &ex));
    if (pg && !(do_fix && P.ns_variant >= 0 && adj_status && K >= T.m)) { g_err = "ce_vjp_params: internal, the factor mode is not available"; return CE_E_STATE; }
    {
        ProfScope ps(h, 1, st);
        CeBwdArgs ba{};
        ba.fix = fix.cur;
        ba.T = T; ba.nkcap = P.nkcap; ba.ldk = P.ldk; ba.Abm = Abm; ba.x = x; ba.y = y; ba.s = s; ba.dx = dx; ba.dy = dy; ba.dA = dAbm; ba.dq = dq_vals;
        ba.sdqk = sdq_k; ba.sdqb = sdq_b; ba.adj = adj_status; ba.P = P_vals; ba.nnz_p = h->nnz_p; ba.pmap = h->d_pmap.get(); ba.prow = h->d_prow.get(); ba.pcol = h->d_pcol.get();
        ba.p_tri = h->p_tri; ba.dP = dP_vals; ba.gA = gA; ba.gK = gK;
        int lrc;
        h->last_fast = -1;
        if (do_fix && P.ns_variant >= 0) {
            ba.T.lda = T.n;
            ba.dA_factors = factors ? 1 : 0;
            lrc = ce_launch_ns(P.ns_variant, B, P.ns_lds, st, ba, NsNoJvp{});
        } else if (P.bwd_mode == BWD_RT) {
            ba.T.lda = T.n;
            int fast = -1; size_t fast_lds = 0;
            if (P.two_tile && adj_status && !P_vals) {
                if (!h->d_nkmax.get()) { HIPCHK(h->d_nkmax.reserve(1)); HIPCHK(hipHostMalloc(&h->h_nkmax, sizeof(int))); HIPCHK(hipEventCreateWithFlags(&h->nk_ev, hipEventDisableTiming)); }
                if (h->nk_pending && hipEventQuery(h->nk_ev) == hipSuccess) {
                    h->nk_last = *h->h_nkmax; h->nk_pending = false; h->nk_have = true;
                    static const bool nk_debug = getenv("CE_NK_DEBUG") != nullptr;
                    if (nk_debug) fprintf(stderr, "cone_engine: largest adjoint system of the previous call: NK = %d (B = %d)\n", h->nk_last, h->nk_B);
                }
                (void)hipGetLastError();          // (hipErrorNotReady of the query is not an error)
                const int need = (h->nk_have && !h->nk_pending && h->nk_B == B) ? h->nk_last + 8 : (1 << 30);
                for (int v = (P.fast_forced >= 0 ? P.fast_forced : 0); v < P.brt_variant; v++) {      // (a forced tile need only hold the template)
                    const BrtRow &R = BRT_ROWS[v];
                    if (P.fast_forced >= 0 ? !brt_tile_holds(T, v) : !(brt_first_tile_ok(T, v, P.brt_variant) && need <= BGC * R.TJ - 1 && need <= R.BGR * R.TI)) continue;
                    fast = v; fast_lds = brt_lds_bytes(T, v); break;
                }
                if (!h->nk_zeroed) { HIPCHK(hipMemsetAsync(h->d_nkmax.get(), 0, sizeof(int), st)); h->nk_zeroed = true; }      // (first call; afterwards the counter is reset behind the read-back)
                ba.nk_max = h->d_nkmax.get();
            }
            if (fast >= 0) {
                h->last_fast = fast;
                ba.nonfinal = 1;      // (an instance this tile does not hold is the retry launch's business, not yet the list's)
                lrc = ce_launch_bwd_rt_plain(fast, B, fast_lds, st, ba);
                ba.retry = 1; ba.nonfinal = 0;
                if (!lrc) lrc = ce_launch_bwd_rt_plain(P.brt_variant, B, P.bwd_lds, st, ba);
            } else
            lrc = (T.ns > 0 || T.nep + T.np > 0) ? ce_launch_bwd_rt_psd(P.brt_variant, B, P.bwd_lds, st, ba) : ce_launch_bwd_rt_plain(P.brt_variant, B, P.bwd_lds, st, ba);
        } else lrc = ce_launch_bwd_generic(P.bwd_mode, B, P.bwd_lds, st, ba);
        if (lrc) { g_err = "internal: no backward kernel for the planned variant"; return CE_E_BADARG; }
        if (do_fix) {
            rc = resolve_run(h, B, fix, [&](int grid, const int *sel, int status_or, int *sel_reset) {
                return vjp_lsqr_launch(h, grid, Abm, K, 1, h->call_q, h->call_sqk, h->call_sqb, x, y, s, dx, dy, dAbm, dq_vals, sdq_k, sdq_b, adj_status, nullptr,
                                       h->rs_atol, h->rs_btol, h->rs_conlim, h->rs_iter_lim, stream, sel, status_or, sel_reset);
            });
            if (rc) return rc;
        }
        if (ba.nk_max) {      // the largest system of this call, for the tile choice of the next one (read once the copy has landed: no synchronisation here)
            HIPCHK(hipMemcpyAsync(h->h_nkmax, h->d_nkmax.get(), sizeof(int), hipMemcpyDeviceToHost, st));
            HIPCHK(hipEventRecord(h->nk_ev, st));
            HIPCHK(hipMemsetAsync(h->d_nkmax.get(), 0, sizeof(int), st));          // for the next call (kept off the path in front of its kernel)
            h->nk_pending = true; h->nk_B = B;
        }
    }
    if (pg) {
        ProfScope ps(h, 2, st);
        CeParamGradArgs ga = *pg;
        ga.rec = dAbm; ga.rpitch = K; ga.srk = 0;
        if (ce_launch_param_grad(st, ga)) { g_err = "ce_vjp_params: the factors of two instances exceed LDS"; return CE_E_TOO_LARGE; }
    }
    if (need_tr) {
        ProfScope ps(h, 2, st);
        if (factors)
            hipLaunchKernelGGL(k_expand_dA, dim3((B + EXP_TB - 1) / EXP_TB, ex.slabs), dim3(EXP_NT), ex.lds, st, T.n, T.m, K, B, ex.slab, T.rowidx, T.colidx, x, y,
                               dAbm, (long)K, dq_vals, sdq_k, sdq_b, adj_status, dA_vals);
        else launch_transpose(st, dAbm, dA_vals, B, K);
    }
    HIPCHK(hipGetLastError());
    return flush_dispatch_order(h, st, nullptr, nullptr);
}

// K cotangents at one solution (include/cone_engine.h).  One launch of k_backward_ns<..., MANY> factors every instance once and writes all K answers; the instances
// it lists as rank deficient are listed ONCE, and ONE launch of the LSQR kernel walks the K x list (cotangent, instance) pairs (SaWalkMany).  The list parity flips once.
// Without an armed re-solve (q_vals == NULL, ce_set_adjoint_resolve(h, 0)) ce_vjp itself does not run the elimination: K calls of it then, the same rule.
// (kind NS_MANY_TRI: ce_vjp_tri_many -- the same body on the triples' variant and footprint; NS_MANY_PSD: ce_vjp_psd_many -- on the PSD blocks'; `who` names the
// entry point in the messages)
enum NsManyKind { NS_MANY_PLAIN = 0, NS_MANY_TRI = 1, NS_MANY_PSD = 2, NS_MANY_PSD_TRI = 3 };          // (NS_MANY_PSD_TRI: ce_vjp_psd_tri_many / ce_jvp_psd_tri_many -- on the row with both kinds' segments)
static int vjp_many_run(ce_handle h, NsManyKind kind, const char *who, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                        const double *x, const double *y, const double *s, const double *dx, const double *dy,
                        double *dA_vals, double *dq_vals, int *adj_status, void *stream, double *rec = nullptr, long rpitch = 0) {
    // rec (ce_vjp_many_params, the plain kind with an armed re-solve): both kernels store the pairs' factor records [K][B][rpitch] instead of dA rows; dA_vals is unused
    const CePlan &P = h->plan;
    const DevT &T = h->T;
    if (B > 1 && sA_b != T.nnz_aug) { g_err = std::string(who) + ": A_vals_bm must be contiguous batch-major rows"; return CE_E_BADARG; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t n = T.n, m = T.m, nnz = T.nnz_aug;
    long syk = (long)((size_t)B * m);
    if (!dy) {
        HIPCHK(h->d_dy0.reserve((size_t)B * m));
        HIPCHK(hipMemsetAsync(h->d_dy0.get(), 0, sizeof(double) * (size_t)B * m, st));
        dy = h->d_dy0.get(); syk = 0;
    }
    NsMany W{K, (long)((size_t)B * n), syk, (long)((size_t)B * nnz), (long)((size_t)B * (n + 1)), (long)B};
    if (rec) { W.rec = rec; W.rpitch = rpitch; W.srk = (long)((size_t)B * rpitch); dA_vals = rec; }          // (a non-null dA for the launchers' checks: neither kernel writes through it)
    if (!(h->resolve && q_vals)) {
        for (int k = 0; k < K; k++) {
            const int rc = ce_vjp(h, B, A_vals_bm, 1, (long)nnz, q_vals, sq_k, sq_b, x, y, s, dx + k * W.sxk, dy + k * W.syk, dA_vals + k * W.sAk, 1, (long)nnz,
                                  dq_vals + k * W.sqk, 1, (long)(n + 1), adj_status ? adj_status + k * W.sak : nullptr, stream);
            if (rc) return rc;
        }
        return CE_OK;
    }
    FixLists fix{nullptr, nullptr};
    int rc = resolve_lists(h, B, st, &fix);
    if (rc) return rc;
    ProfScope ps(h, 1, st);
    CeBwdArgs ba{};
    ba.T = T; ba.T.lda = T.n; ba.Abm = A_vals_bm; ba.x = x; ba.y = y; ba.s = s; ba.dx = dx; ba.dy = dy; ba.dA = dA_vals; ba.dq = dq_vals; ba.sdqk = 1; ba.sdqb = (long)(n + 1);
    ba.adj = adj_status; ba.fix = fix.cur;
    h->last_fast = -1;
    if (kind == NS_MANY_PSD_TRI ? ce_launch_ns(P.psd_tri_ns_variant, B, P.psd_tri_ns_lds, st, ba, NsVjpManyPsdTri{W})
        : kind == NS_MANY_PSD ? ce_launch_ns(P.psd_ns_variant, B, P.psd_ns_lds, st, ba, NsVjpManyPsd{W})
        : kind == NS_MANY_TRI ? ce_launch_ns(P.tri_ns_variant, B, P.tri_ns_lds, st, ba, NsVjpTriMany{W}) : ce_launch_ns(P.ns_variant, B, P.ns_lds, st, ba, W)) {
        g_err = "internal: no many-cotangent kernel for the planned variant"; return CE_E_BADARG;
    }
    const int grid = B < 768 ? B : 768;          // (resolve_run's grid)
    const int prof_keep = h->prof; h->prof = 0;
    SaWalkMany wm; wm.K = K; wm.sxk = W.sxk; wm.syk = W.syk; wm.sAk = W.sAk; wm.sqk = W.sqk; wm.sak = W.sak; wm.rec = W.rec; wm.rpitch = W.rpitch; wm.srk = W.srk;
    rc = vjp_lsqr_launch(h, grid, A_vals_bm, (long)nnz, 1, q_vals, sq_k, sq_b, x, y, s, dx, dy, dA_vals, dq_vals, 1, (long)(n + 1),
                         adj_status, nullptr, h->rs_atol, h->rs_btol, h->rs_conlim, h->rs_iter_lim, stream, fix.cur, 4 | 8, fix.oth, nullptr, &wm);
    h->fix_par ^= 1;
    h->prof = prof_keep;
    if (rc) return rc;
    HIPCHK(hipGetLastError());
    return CE_OK;
}
int ce_vjp_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                const double *x, const double *y, const double *s, const double *dx, const double *dy,
                double *dA_vals, double *dq_vals, int *adj_status, void *stream) {
    if (!h || B <= 0 || K <= 0 || !A_vals_bm || !x || !y || !s || !dx || !dA_vals || !dq_vals) { g_err = "ce_vjp_many: null argument, B <= 0 or K <= 0"; return CE_E_BADARG; }
    if (ce_vjp_many_variant(h) < 0) {
        g_err = "ce_vjp_many: this template has no many-cotangent elimination (PSD / exponential / power cones, a quadratic objective inside the kernels, n > 108, "
                "CE_BWD_NS=0, or the LSQR vectors of the re-solve exceed LDS); call ce_vjp once per cotangent";
        return CE_E_UNSUPPORTED;
    }
    return vjp_many_run(h, NS_MANY_PLAIN, "ce_vjp_many", B, K, A_vals_bm, sA_b, q_vals, sq_k, sq_b, x, y, s, dx, dy, dA_vals, dq_vals, adj_status, stream);
}
// The parameter gradients of K cotangents at one solution, no dA (include/cone_engine.h): ce_vjp_many's two launches in record mode -- the elimination and the LSQR
// walk leave (r_y, r_tau, r_x) per pair in d_rec -- and k_param_grad behind them, which applies the composed transposed parameter maps to the entries it
// evaluates from the records.  The pitch m + 1 + n keeps r_x beside r_y: a re-solved pair's r_x is NOT x r_tau - dq to the last bit, and the entries are to be
// the ones the dA route stores.
static const char *const PG_REFUSAL = ": this template has no parameter gradient from the factors (ce_param_grad_variant < 0: PSD / exponential / power cones, a quadratic "
                                      "objective inside the kernels, n > 108, CE_BWD_NS=0, or the LSQR vectors of the re-solve exceed LDS); use the dA entry points";
// (served / refusal: the entry's own condition -- ce_param_grad_variant for the plain kind, the kind's many-cotangent variant for the others; need_resolve: every
// kind but the QP one, which has no re-solve behind its launch)
static int pg_check(ce_handle h, const char *who, int rows, const int *map_ptr, const int *map_code, const int *map_k, const double *map_val, const double *q_vals,
                    int served = -2, const char *refusal = nullptr, bool need_resolve = true) {
    if (rows <= 0 || !map_ptr || !map_code || !map_k || !map_val) { g_err = std::string(who) + ": null map argument or rows <= 0"; return CE_E_BADARG; }
    if (served == -2) { served = ce_param_grad_variant(h); refusal = PG_REFUSAL; }
    if (served < 0 || h->T.m >= (1 << 16)) { g_err = std::string(who) + refusal; return CE_E_UNSUPPORTED; }
    if (need_resolve && !(h->resolve && q_vals)) { g_err = std::string(who) + ": the re-solve must be armed (q_vals given, ce_set_adjoint_resolve enabled): the factor modes run in front of it alone"; return CE_E_UNSUPPORTED; }
#ifdef CE_TIMING
    g_err = std::string(who) + ": not available in the timing build (its stamps go to the dA rows)"; return CE_E_UNSUPPORTED;
#endif
    return CE_OK;
}
// k_param_grad behind a record-mode launch of any kind: the records of the call in d_rec, the pairs' dq rows where the adjoint wrote them
static int pg_records_launch(ce_handle h, const std::string &who, int B, int K, const double *x, const double *y, int rows, const int *map_ptr, const int *map_code,
                             const int *map_k, const double *map_val, double *g, const double *dq_vals, const int *adj_status, void *stream) {
    const DevT &T = h->T;
    const long rpitch = (long)T.m + 1 + T.n;
    CeParamGradArgs ga{T.n, T.m, B, K, rows, 0, PG_RECORDS, map_ptr, map_code, map_k, map_val, x, y, dq_vals, (long)((size_t)B * (T.n + 1)), 1, (long)(T.n + 1),
                       h->d_rec.get(), rpitch, (long)((size_t)B * rpitch), adj_status, g};
    {
        ProfScope ps(h, 2, (hipStream_t)stream);
        if (ce_launch_param_grad((hipStream_t)stream, ga)) { g_err = who + ": the factors of two pairs exceed LDS"; return CE_E_TOO_LARGE; }
    }
    HIPCHK(hipGetLastError());
    return CE_OK;
}
// the body of ce_vjp_many_params and of its TRI / PSD / PSD + TRI twins: `served` is the kind's many-cotangent variant (-2: the plain kind's ce_param_grad_variant)
static int vjp_many_params_run(ce_handle h, NsManyKind kind, const char *who, int served, const char *refusal, int B, int K, const double *A_vals_bm, long sA_b,
                               const double *q_vals, long sq_k, long sq_b, const double *x, const double *y, const double *s, const double *dx, const double *dy,
                               int rows, const int *map_ptr, const int *map_code, const int *map_k, const double *map_val,
                               double *g, double *dq_vals, int *adj_status, void *stream) {
    if (!h || B <= 0 || K <= 0 || !A_vals_bm || !x || !y || !s || !dx || !g || !dq_vals || !adj_status) { g_err = std::string(who) + ": null argument, B <= 0 or K <= 0"; return CE_E_BADARG; }
    int rc = pg_check(h, who, rows, map_ptr, map_code, map_k, map_val, q_vals, served, refusal);
    if (rc) return rc;
    const DevT &T = h->T;
    const long rpitch = (long)T.m + 1 + T.n;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(h->d_rec.reserve((size_t)K * B * rpitch));
    rc = vjp_many_run(h, kind, who, B, K, A_vals_bm, sA_b, q_vals, sq_k, sq_b, x, y, s, dx, dy, nullptr, dq_vals, adj_status, stream, h->d_rec.get(), rpitch);
    if (rc) return rc;
    return pg_records_launch(h, who, B, K, x, y, rows, map_ptr, map_code, map_k, map_val, g, dq_vals, adj_status, stream);
}
int ce_vjp_many_params(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                       const double *x, const double *y, const double *s, const double *dx, const double *dy,
                       int rows, const int *map_ptr, const int *map_code, const int *map_k, const double *map_val,
                       double *g, double *dq_vals, int *adj_status, void *stream) {
    return vjp_many_params_run(h, NS_MANY_PLAIN, "ce_vjp_many_params", -2, nullptr, B, K, A_vals_bm, sA_b, q_vals, sq_k, sq_b, x, y, s, dx, dy, rows, map_ptr, map_code, map_k, map_val,
                               g, dq_vals, adj_status, stream);
}
// The same for the other many-cotangent kinds (include/cone_engine.h): each is served exactly where its kind's ce_vjp_*_many_variant >= 0 and refuses every other
// handle -- a plain one included -- before anything is enqueued.  The records are the plain kind's: r_y stands in the original basis behind the triples' / blocks' rotation.
int ce_vjp_tri_many_params(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                           const double *x, const double *y, const double *s, const double *dx, const double *dy,
                           int rows, const int *map_ptr, const int *map_code, const int *map_k, const double *map_val,
                           double *g, double *dq_vals, int *adj_status, void *stream) {
    return vjp_many_params_run(h, NS_MANY_TRI, "ce_vjp_tri_many_params", ce_vjp_tri_many_variant(h),
                               ": this template has no search-free elimination with triples (ce_vjp_tri_many_variant < 0); use the dA entry points, or the *_many_params entry of its kind",
                               B, K, A_vals_bm, sA_b, q_vals, sq_k, sq_b, x, y, s, dx, dy, rows, map_ptr, map_code, map_k, map_val, g, dq_vals, adj_status, stream);
}
int ce_vjp_psd_many_params(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                           const double *x, const double *y, const double *s, const double *dx, const double *dy,
                           int rows, const int *map_ptr, const int *map_code, const int *map_k, const double *map_val,
                           double *g, double *dq_vals, int *adj_status, void *stream) {
    return vjp_many_params_run(h, NS_MANY_PSD, "ce_vjp_psd_many_params", ce_vjp_psd_many_variant(h),
                               ": this template has no search-free elimination with PSD blocks (ce_vjp_psd_many_variant < 0); use the dA entry points, or the *_many_params entry of its kind",
                               B, K, A_vals_bm, sA_b, q_vals, sq_k, sq_b, x, y, s, dx, dy, rows, map_ptr, map_code, map_k, map_val, g, dq_vals, adj_status, stream);
}
int ce_vjp_psd_tri_many_params(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                               const double *x, const double *y, const double *s, const double *dx, const double *dy,
                               int rows, const int *map_ptr, const int *map_code, const int *map_k, const double *map_val,
                               double *g, double *dq_vals, int *adj_status, void *stream) {
    return vjp_many_params_run(h, NS_MANY_PSD_TRI, "ce_vjp_psd_tri_many_params", ce_vjp_psd_tri_many_variant(h),
                               ": this template has no search-free elimination with PSD blocks and triples (ce_vjp_psd_tri_many_variant < 0); use the dA entry points, or the *_many_params entry of its kind",
                               B, K, A_vals_bm, sA_b, q_vals, sq_k, sq_b, x, y, s, dx, dy, rows, map_ptr, map_code, map_k, map_val, g, dq_vals, adj_status, stream);
}
// the factor records the last ce_vjp_many_params call of this (B, K) left in the engine's workspace, [K][B][m + 1 + n], copied to `out` on the stream (introspection
// for tests: r_tau of a pair is not observable from g and dq)
int ce_param_grad_records(ce_handle h, int B, int K, double *out, void *stream) {
    if (!h || B <= 0 || K <= 0 || !out) { g_err = "ce_param_grad_records: null argument, B <= 0 or K <= 0"; return CE_E_BADARG; }
    const size_t cnt = (size_t)K * B * ((size_t)h->T.m + 1 + h->T.n);
    if (!h->d_rec.get() || h->d_rec.capacity() < cnt) { g_err = "ce_param_grad_records: no *_many_params call of this size has run"; return CE_E_STATE; }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(out, h->d_rec.get(), sizeof(double) * cnt, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return CE_OK;
}
// One cotangent: the single-cotangent adjoint in its factor mode (r_y at the head of the instance's workspace row, the whole row of a re-solved instance -- today's
// convention, the NsNoJvp kernel untouched) and k_param_grad in its row-head mode behind it.  K = 1 of the many-mode loses to ce_vjp (README), hence an entry of its own.
int ce_vjp_params(ce_handle h, int B, const double *A_vals, long sA_k, long sA_b, const double *q_vals, long sq_k, long sq_b,
                  const double *x, const double *y, const double *s, const double *dx, const double *dy,
                  int rows, const int *map_ptr, const int *map_code, const int *map_k, const double *map_val,
                  double *g, double *dq_vals, long sdq_k, long sdq_b, int *adj_status, void *stream) {
    if (!h || B <= 0 || !x || !y || !s || !dx || !dy || !g || !dq_vals || !adj_status) { g_err = "ce_vjp_params: null argument or B <= 0"; return CE_E_BADARG; }
    int rc = pg_check(h, "ce_vjp_params", rows, map_ptr, map_code, map_k, map_val, q_vals);
    if (rc) return rc;
    const DevT &T = h->T;
    if (T.nnz_aug < T.m) { g_err = "ce_vjp_params: a value row shorter than m cannot hold the factors (nnz_aug < m); call ce_vjp_many_params with K = 1"; return CE_E_UNSUPPORTED; }
    const CeParamGradArgs ga{T.n, T.m, B, 1, rows, 0, PG_ROWHEAD, map_ptr, map_code, map_k, map_val, x, y, dq_vals, 0, sdq_k, sdq_b, nullptr, 0, 0, adj_status, g};
    h->pg = &ga; h->call_q = q_vals; h->call_sqk = sq_k; h->call_sqb = sq_b;
    rc = ce_vjp_qp(h, B, A_vals, sA_k, sA_b, nullptr, x, y, s, dx, dy, nullptr, 0, 0, dq_vals, sdq_k, sdq_b, nullptr, adj_status, stream);
    h->pg = nullptr; h->call_q = nullptr;
    return rc;
}
// K cotangents at one solution of a template with exponential / power triples (include/cone_engine.h): ce_vjp_many's body with k_backward_ns<..., TRI, MANY> on the
// triples' variant and footprint.  Without an armed re-solve K calls of ce_vjp, whose pivoting kernel serves such templates.
int ce_vjp_tri_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                    const double *x, const double *y, const double *s, const double *dx, const double *dy,
                    double *dA_vals, double *dq_vals, int *adj_status, void *stream) {
    if (!h || B <= 0 || K <= 0 || !A_vals_bm || !x || !y || !s || !dx || !dA_vals || !dq_vals) { g_err = "ce_vjp_tri_many: null argument, B <= 0 or K <= 0"; return CE_E_BADARG; }
    if (ce_vjp_tri_many_variant(h) < 0) {
        g_err = "ce_vjp_tri_many: this template has no search-free elimination with triples (no exponential / power cone, PSD cones, a quadratic objective inside the "
                "kernels, n > 108, CE_BWD_NS=0, or the LSQR vectors of the re-solve exceed LDS); call ce_vjp_many or ce_vjp";
        return CE_E_UNSUPPORTED;
    }
    return vjp_many_run(h, NS_MANY_TRI, "ce_vjp_tri_many", B, K, A_vals_bm, sA_b, q_vals, sq_k, sq_b, x, y, s, dx, dy, dA_vals, dq_vals, adj_status, stream);
}
// K cotangents at one solution of a template with PSD blocks (include/cone_engine.h): ce_vjp_many's body with k_backward_ns<..., MANY, PSD> on the blocks' variant and
// footprint.  Without an armed re-solve K calls of ce_vjp, whose pivoting kernel serves such templates.
int ce_vjp_psd_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                    const double *x, const double *y, const double *s, const double *dx, const double *dy,
                    double *dA_vals, double *dq_vals, int *adj_status, void *stream) {
    if (!h || B <= 0 || K <= 0 || !A_vals_bm || !x || !y || !s || !dx || !dA_vals || !dq_vals) { g_err = "ce_vjp_psd_many: null argument, B <= 0 or K <= 0"; return CE_E_BADARG; }
    if (ce_vjp_psd_many_variant(h) < 0) {
        g_err = "ce_vjp_psd_many: this template has no search-free elimination with PSD blocks (no PSD block, triples or a quadratic objective beside them, n > 108, "
                "its footprint exceeds LDS, or CE_BWD_NS=0); call ce_vjp once per cotangent";
        return CE_E_UNSUPPORTED;
    }
    return vjp_many_run(h, NS_MANY_PSD, "ce_vjp_psd_many", B, K, A_vals_bm, sA_b, q_vals, sq_k, sq_b, x, y, s, dx, dy, dA_vals, dq_vals, adj_status, stream);
}
// K cotangents at one solution of a template with PSD blocks AND exponential / power triples (include/cone_engine.h): ce_vjp_many's body with
// k_backward_ns<..., TRI, MANY, PSD> on the variant and footprint with both kinds' segments.  Without an armed re-solve K calls of ce_vjp.
int ce_vjp_psd_tri_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                        const double *x, const double *y, const double *s, const double *dx, const double *dy,
                        double *dA_vals, double *dq_vals, int *adj_status, void *stream) {
    if (!h || B <= 0 || K <= 0 || !A_vals_bm || !x || !y || !s || !dx || !dA_vals || !dq_vals) { g_err = "ce_vjp_psd_tri_many: null argument, B <= 0 or K <= 0"; return CE_E_BADARG; }
    if (ce_vjp_psd_tri_many_variant(h) < 0) {
        g_err = "ce_vjp_psd_tri_many: this template has no search-free elimination with PSD blocks and triples (it lacks a PSD block or an exponential / power cone, "
                "has a quadratic objective, n > 108, its footprint exceeds LDS, or CE_BWD_NS=0); call ce_vjp once per cotangent";
        return CE_E_UNSUPPORTED;
    }
    return vjp_many_run(h, NS_MANY_PSD_TRI, "ce_vjp_psd_tri_many", B, K, A_vals_bm, sA_b, q_vals, sq_k, sq_b, x, y, s, dx, dy, dA_vals, dq_vals, adj_status, stream);
}

// summary of an int32 vector v[B] (status of a forward call, or adj_status of a backward call): out[0] = min v, out[1] = #{v == 2} ("solved,
// inaccurate"), out[2] = #{(v & 3) != 0} (adjoint flags: bits 0-1 = failed / too many active rows): what a caller needs to decide whether
// the slow path (per-instance inspection, messages) is necessary at all
__global__ void __launch_bounds__(256) k_status_summary(int B, const int *__restrict__ status, int *__restrict__ out) {
    int mn = 0x7fffffff, n2 = 0, nf = 0;
    for (int i = threadIdx.x; i < B; i += 256) { const int s = status[i]; mn = min(mn, s); n2 += (s == 2); nf += ((s & 3) != 0); }
    for (int o = 32; o > 0; o >>= 1) { mn = min(mn, __shfl_xor(mn, o)); n2 += __shfl_xor(n2, o); nf += __shfl_xor(nf, o); }
    __shared__ int sm[12];
    if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6] = mn; sm[4 + (threadIdx.x >> 6)] = n2; sm[8 + (threadIdx.x >> 6)] = nf; }
    __syncthreads();
    if (threadIdx.x == 0) {
        out[0] = min(min(sm[0], sm[1]), min(sm[2], sm[3])); out[1] = sm[4] + sm[5] + sm[6] + sm[7]; out[2] = sm[8] + sm[9] + sm[10] + sm[11];
        __threadfence_system();          // (out may be mapped host memory: the three values are visible to the host before the flag)
        __hip_atomic_store(out + 3, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);      // out[3] = 1: "ready" -- a host that cleared it before the call may poll it instead of synchronising the stream
    }
}
// order[] = the instances sorted by iteration count, largest first (counting sort over check intervals; ties in arbitrary order): one workgroup.
// order[B] = 1 when the history is PREDICTIVE: at least 70 % of the instances stopped in the same check interval as the instance at the same position of the call
// before (iters_prev, updated here; have_prev = 0: no such call).  Re-solved or slowly changing batches score ~1, unrelated batches of the metric configuration
// ~0.43 (the chance that two draws of the count distribution agree): there the permutation predicts nothing and is not applied (k_fwd2 reads the flag).
// sum_status / sum_out given: the status summary of k_status_summary comes FIRST (its ready flag is what the host polls), the sort behind it in the same launch
__global__ void __launch_bounds__(1024) k_dispatch_order(int B, const int *__restrict__ iters, int *__restrict__ order, int *__restrict__ iters_prev, int have_prev,
                                                         const int *__restrict__ sum_status = nullptr, int *__restrict__ sum_out = nullptr) {
    constexpr int NB = 512;                       // buckets of CONVERGED_INTERVAL iterations; anything longer shares the last one
    __shared__ int cnt[NB], tmp[NB];
    __shared__ int same;
    if (sum_out) {
        int mn = 0x7fffffff, n2 = 0, nf = 0;
        for (int i = threadIdx.x; i < B; i += 1024) { const int s = sum_status[i]; mn = min(mn, s); n2 += (s == 2); nf += ((s & 3) != 0); }
        for (int o = 32; o > 0; o >>= 1) { mn = min(mn, __shfl_xor(mn, o)); n2 += __shfl_xor(n2, o); nf += __shfl_xor(nf, o); }
        if ((threadIdx.x & 63) == 0) { tmp[threadIdx.x >> 6] = mn; tmp[16 + (threadIdx.x >> 6)] = n2; tmp[32 + (threadIdx.x >> 6)] = nf; }
        __syncthreads();
        if (threadIdx.x == 0) {
            int a = tmp[0], b2 = 0, c = 0;
            for (int w = 0; w < 16; w++) { a = min(a, tmp[w]); b2 += tmp[16 + w]; c += tmp[32 + w]; }
            sum_out[0] = a; sum_out[1] = b2; sum_out[2] = c;
            __threadfence_system();
            __hip_atomic_store(sum_out + 3, 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) same = 0;
    for (int b = threadIdx.x; b < NB; b += 1024) cnt[b] = 0;
    __syncthreads();
    {
        int mine = 0;
        for (int i = threadIdx.x; i < B; i += 1024) {
            const int it = iters[i];
            if (have_prev) mine += (max(it, 0) / CONVERGED_INTERVAL == max(iters_prev[i], 0) / CONVERGED_INTERVAL);
            iters_prev[i] = it;
        }
        if (have_prev && mine) atomicAdd(&same, mine);
    }
    __syncthreads();
    // not predictive (unrelated batches, the first call): the order would not be applied -- the sort is skipped, the kernel is ~5 us shorter on the path to the caller's next launch
    if (!(have_prev && 10 * same >= 7 * B)) { if (threadIdx.x == 0) order[B] = 0; return; }
    for (int i = threadIdx.x; i < B; i += 1024) { const int b = min(max(iters[i], 0) / CONVERGED_INTERVAL, NB - 1); atomicAdd(&cnt[NB - 1 - b], 1); }      // (bucket 0 = longest)
    __syncthreads();
    // exclusive prefix sum over the buckets (two per thread, log-step scan: a serial loop over 512 LDS entries cost 13 us on the path to the status read-back)
    int *src = cnt, *dst = tmp;
    for (int off = 1; off < NB; off <<= 1) {
        for (int b = threadIdx.x; b < NB; b += 1024) dst[b] = src[b] + (b >= off ? src[b - off] : 0);
        __syncthreads();
        int *t = src; src = dst; dst = t;
    }
    for (int b = threadIdx.x; b < NB; b += 1024) dst[b] = b > 0 ? src[b - 1] : 0;          // inclusive -> exclusive
    __syncthreads();
    for (int i = threadIdx.x; i < B; i += 1024) { const int b = min(max(iters[i], 0) / CONVERGED_INTERVAL, NB - 1); order[atomicAdd(&dst[NB - 1 - b], 1)] = i; }
    if (threadIdx.x == 0) order[B] = 1;
}
// the order of the NEXT solve is computed off the critical path: behind the status summary (the host is busy with autograd then, the device idle), or at the
// latest in front of the next solve / behind the next adjoint
static int flush_dispatch_order(ce_engine *h, hipStream_t st, const int *sum_status = nullptr, int *sum_out = nullptr) {
    if (!h->order_pending_B) return CE_OK;
    const int B = h->order_pending_B;
    h->order_pending_B = 0;
    HIPCHK(h->d_order.reserve((size_t)B + 1));
    if (h->d_iters_prev.capacity() < (size_t)B) h->iters_prev_B = 0;      // (a new buffer holds no history)
    HIPCHK(h->d_iters_prev.reserve(B));
    // (on a stream of the engine's own, ordered by two events, this kernel was measured SLOWER: a cross-queue dependency costs more than the 10 us it would hide -- 2.13 against 2.05 ms
    //  per replayed step, no change on rotating batches)
    hipLaunchKernelGGL(k_dispatch_order, dim3(1), dim3(1024), 0, st, B, h->d_iters2.get(), h->d_order.get(), h->d_iters_prev.get(), h->iters_prev_B == B ? 1 : 0, sum_status, sum_out);
    h->iters_prev_B = B;
    HIPCHK(hipGetLastError());
    h->order_B = B;
    return CE_OK;
}
int ce_set_dispatch_history(ce_handle h, int on) {
    if (!h) { g_err = "null argument"; return CE_E_BADARG; }
    h->dispatch_history = on != 0;
    if (!on) { h->order_B = 0; h->order_pending_B = 0; h->iters_prev_B = 0; }
    return CE_OK;
}

int ce_status_summary(ce_handle h, int B, const int *status, int *summary_host, void *stream) {
    if (!h || B <= 0 || !status || !summary_host) { g_err = "null argument"; return CE_E_BADARG; }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(h->d_summary.reserve(8 * 4));
    // Pinned host memory is mapped into the device's address space: the kernel stores the three ints there itself (no copy kernel behind it: two launches
    // less per step of the plugin).  Anything else (the pointer is checked once and remembered) goes through a device slot and an asynchronous copy.
    const uintptr_t page = (uintptr_t)summary_host & ~(uintptr_t)63;      // (the plugin alternates two slots of one 32-byte pinned buffer: remember the 64-byte line)
    if (page != h->summary_host_checked) {
        hipPointerAttribute_t at; char *dp = nullptr;
        const bool mapped = hipPointerGetAttributes(&at, (void *)page) == hipSuccess && at.type == hipMemoryTypeHost &&
                            hipHostGetDevicePointer((void **)&dp, (void *)page, 0) == hipSuccess && dp != nullptr;
        (void)hipGetLastError();
        h->summary_host_checked = page; h->summary_host_dev = mapped ? dp : nullptr;
    }
    if (h->summary_host_dev) {
        int *out = reinterpret_cast<int *>(h->summary_host_dev + ((uintptr_t)summary_host - page));
        // a solve whose dispatch order is still owed and whose status this is: ONE launch does both, the summary (and its ready flag) first
        if (h->order_pending_B == B && status == h->last_status) return flush_dispatch_order(h, (hipStream_t)stream, status, out);
        hipLaunchKernelGGL(k_status_summary, dim3(1), dim3(256), 0, (hipStream_t)stream, B, status, out);
        HIPCHK(hipGetLastError());
        return flush_dispatch_order(h, (hipStream_t)stream, nullptr, nullptr);          // (behind the summary: the host reads the flag while this runs)
    }
    int *slot = h->d_summary.get() + 4 * (h->summary_next++ & 7);      // a few calls may be in flight on the stream before the caller synchronises
    hipLaunchKernelGGL(k_status_summary, dim3(1), dim3(256), 0, (hipStream_t)stream, B, status, slot);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(summary_host, slot, 4 * sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));      // (three values + the ready flag)
    return flush_dispatch_order(h, (hipStream_t)stream, nullptr, nullptr);
}

int ce_transpose(ce_handle h, int rows, int cols, const double *in, double *out, void *stream) {
    if (!h || !in || !out || rows <= 0 || cols <= 0) { g_err = "null argument"; return CE_E_BADARG; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps(h, 2, st);
        launch_transpose(st, in, out, rows, cols);
    }
    HIPCHK(hipGetLastError());
    return CE_OK;
}

// ---- optimal value and its envelope-theorem derivatives (ce_value.h): launches under profiling class 2 (no system is solved: not the adjoint's family)
static int value_check_p(const void *vals, const int *p_rows, const int *p_cols, int nnz_p, bool need_vals) {
    if (nnz_p < 0 || (nnz_p > 0 && (!p_rows || !p_cols || (need_vals && !vals)))) { g_err = "quadratic objective: nnz_p > 0 needs the values and p_rows, p_cols (device arrays)"; return CE_E_BADARG; }
    return CE_OK;
}
static int value_launch(ce_handle h, bool jvp, CeValueArgs &a, const int *p_rows, const int *p_cols, int nnz_p, void *stream) {
    const DevT &T = h->T;
    a.n = T.n; a.m = T.m; a.nnz_aug = T.nnz_aug; a.nnz_p = nnz_p;
    a.rowidx = h->d_rowidx.get(); a.colidx = h->d_colidx.get(); a.bpos = h->d_bpos.get(); a.prow = p_rows; a.pcol = p_cols;
    const size_t lds = ce_value_lds(T.n, T.m);
    if (lds > VALUE_LDS_MAX) { g_err = "ce_value: x and y of one instance exceed LDS"; return CE_E_TOO_LARGE; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps(h, 2, st);
        ce_launch_value(jvp, lds, st, a);
    }
    HIPCHK(hipGetLastError());
    return CE_OK;
}
int ce_value(ce_handle h, int B, const double *A_vals, long sA_k, long sA_b, const double *q_vals, long sq_k, long sq_b,
             const double *P_vals, const int *p_rows, const int *p_cols, int nnz_p, const double *x, const double *y, double *pobj, double *dobj, void *stream) {
    if (!h || B <= 0 || !A_vals || !q_vals || !x || !y || !pobj || !dobj) { g_err = "null argument"; return CE_E_BADARG; }
    const int rc = value_check_p(P_vals, p_rows, p_cols, nnz_p, true);
    if (rc) return rc;
    CeValueArgs a{};
    a.B = B; a.x = x; a.y = y; a.A = A_vals; a.sAk = sA_k; a.sAb = sA_b; a.q = q_vals; a.sqk = sq_k; a.sqb = sq_b; a.P = P_vals; a.pobj = pobj; a.dobj = dobj;
    return value_launch(h, false, a, p_rows, p_cols, nnz_p, stream);
}
int ce_value_jvp(ce_handle h, int B, const double *tA_vals_bm, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                 const double *tP_vals, const int *p_rows, const int *p_cols, int nnz_p, const double *x, const double *y, double *tval, void *stream) {
    if (!h || B <= 0 || !x || !y || !tval) { g_err = "null argument"; return CE_E_BADARG; }
    const int rc = value_check_p(tP_vals, p_rows, p_cols, tP_vals ? nnz_p : 0, false);
    if (rc) return rc;
    if (tA_vals_bm && B > 1 && stA_b < h->T.nnz_aug) { g_err = "ce_value_jvp: tA_vals_bm must be batch-major rows at least nnz_aug apart"; return CE_E_BADARG; }
    CeValueArgs a{};
    a.B = B; a.x = x; a.y = y; a.tA = tA_vals_bm; a.stAb = stA_b; a.tq = tq_vals; a.stqk = stq_k; a.stqb = stq_b; a.tP = tP_vals; a.tval = tval;
    return value_launch(h, true, a, p_rows, p_cols, tP_vals ? nnz_p : 0, stream);
}
int ce_value_vjp(ce_handle h, int B, const double *x, const double *y, const double *g, const unsigned char *skip,
                 double *dA_vals, long sdA_k, long sdA_b, double *dq_vals, long sdq_k, long sdq_b,
                 double *dP_vals, const int *p_rows, const int *p_cols, int nnz_p, void *stream) {
    if (!h || B <= 0 || !x || !y || !g) { g_err = "null argument"; return CE_E_BADARG; }
    int rc = value_check_p(dP_vals, p_rows, p_cols, dP_vals ? nnz_p : 0, false);
    if (rc) return rc;
    const DevT &T = h->T;
    const int K = T.nnz_aug;
    const bool rows = dA_vals && sdA_k == 1 && (sdA_b >= K || B == 1), tile = dA_vals && !rows && sdA_b == 1 && sdA_k >= B;
    if (dA_vals && !rows && !tile) { g_err = "dA_vals must be batch-minor (sdA_k >= B, sdA_b = 1) or batch-major (sdA_k = 1, sdA_b >= nnz_aug)"; return CE_E_BADARG; }
    CeValueVjpArgs a{};
    a.B = B; a.n = T.n; a.m = T.m; a.nnz_aug = K; a.nnz_p = dP_vals ? nnz_p : 0;
    a.rowidx = h->d_rowidx.get(); a.colidx = h->d_colidx.get(); a.prow = p_rows; a.pcol = p_cols;
    a.x = x; a.y = y; a.g = g; a.skip = skip;
    a.dA = dA_vals; a.sdAk = sdA_k; a.sdAb = sdA_b; a.dq = dq_vals; a.sdqk = sdq_k; a.sdqb = sdq_b; a.dP = dP_vals;
    const size_t lds_rows = ce_value_vjp_rows_lds(T.n, T.m), lds_tile = ce_value_vjp_tile_lds(T.n, T.m);
    if (lds_rows > VALUE_LDS_MAX) { g_err = "ce_value_vjp: x and y of four instances exceed LDS"; return CE_E_TOO_LARGE; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps(h, 2, st);
        const bool tile_dq = tile && dq_vals && sdq_b == 1;      // (the tile kernel stores dq coalesced in that layout)
        if (tile) {
            // chunks of entries per tile: enough workgroups to fill the device at small tile counts, never below 256 entries (each workgroup stages its tile again)
            const int tiles = (B + 63) / 64;
            const int chunks = std::max(1, std::min((1024 + tiles - 1) / tiles, (K + 255) / 256));
            const int kchunk = (K + chunks - 1) / chunks;
            ce_launch_value_vjp_tile(lds_tile <= VALUE_LDS_MAX, chunks, kchunk, tile_dq ? 1 : 0, lds_tile, st, a);
        }
        CeValueVjpArgs r = a;
        if (tile) r.dA = nullptr;
        if (tile_dq) r.dq = nullptr;
        if (r.dA || r.dq || r.dP) ce_launch_value_vjp_rows(lds_rows, st, r);
    }
    HIPCHK(hipGetLastError());
    return CE_OK;
}

// ---- the termination test at a given point (ce_check.h): one launch per instance set + one that counts, under profiling class 2
static constexpr size_t CHECK_STAGE_MAX = 64 * 1024;      // the value row is staged in LDS while two workgroups still share a CU; beyond, it is read twice (L2)
static int check_group(int rows) { int g = 1; while (2 * g * rows <= 256 && g < 64) g *= 2; return g; }      // threads per row: the largest power of two with g * rows <= 256
int ce_check_solved(ce_handle h, int B, const double *A_vals, long sA_k, long sA_b, const double *q_vals, long sq_k, long sq_b,
                    const double *P_vals, const int *p_rows, const int *p_cols, int nnz_p,
                    const double *x, const double *y, const double *s, const int *eligible, int eligible_mask, double eps_abs, double eps_rel,
                    unsigned char *solved, int *status, int *iters, double *resid, int *n_unsolved, void *stream) {
    if (!h || B <= 0 || !A_vals || !q_vals || !x || !y || !s || !solved || !status || !iters || !resid || !n_unsolved) { g_err = "null argument"; return CE_E_BADARG; }
    const int rc = value_check_p(P_vals, p_rows, p_cols, nnz_p, true);
    if (rc) return rc;
    const DevT &T = h->T;
    CeCheckArgs a{};
    a.B = B; a.n = T.n; a.m = T.m; a.nnz_aug = T.nnz_aug; a.nnz_p = P_vals ? nnz_p : 0; a.gr = check_group(T.m); a.gc = check_group(T.n);
    a.rptr = h->d_csr_ptr.get(); a.rcol = h->d_csr_col.get(); a.rsrc = h->d_csr_src.get(); a.cptr = h->d_csc_ptr.get(); a.rowidx = h->d_rowidx.get(); a.bpos = h->d_bpos.get();
    a.prow = p_rows; a.pcol = p_cols;
    a.A = A_vals; a.sAk = sA_k; a.sAb = sA_b; a.q = q_vals; a.sqk = sq_k; a.sqb = sq_b; a.P = P_vals;
    a.x = x; a.y = y; a.s = s; a.eligible = eligible; a.emask = eligible_mask; a.eps_abs = eps_abs; a.eps_rel = eps_rel;
    a.solved = solved; a.status = status; a.iters = iters; a.resid = resid;
    const size_t lds0 = ce_check_lds(T.n, T.m, 0), lds1 = ce_check_lds(T.n, T.m, T.nnz_aug);
    if (lds0 > VALUE_LDS_MAX) { g_err = "ce_check_solved: x, y, s and the products of one instance exceed LDS"; return CE_E_TOO_LARGE; }
    const bool staged = lds1 <= CHECK_STAGE_MAX;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps(h, 2, st);
        ce_launch_check_solved(staged, staged ? lds1 : lds0, st, a, n_unsolved);
    }
    HIPCHK(hipGetLastError());
    return CE_OK;
}

// ---- LPGD backward (ce_lpgd.h): the perturbed data of one side and the differenced envelope gradients; streaming passes under profiling class 2
int ce_set_transient_solve(ce_handle h, int on) {
    if (!h) { g_err = "null argument"; return CE_E_BADARG; }
    h->transient_solve = on != 0;
    return CE_OK;
}
int ce_lpgd_perturb(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                    const double *P_vals, const int *p_rows, const int *p_cols, int nnz_p,
                    const double *x, const double *dx, const double *dy, double tau, double rho,
                    double *q_out, double *A_out_bm, double *P_out, int *flags, void *stream) {
    if (!h || B <= 0 || !q_vals || !x || !dx || !q_out || !flags) { g_err = "null argument"; return CE_E_BADARG; }
    if (!(tau != 0.0) || !(rho >= 0.0)) { g_err = "ce_lpgd_perturb: tau must be nonzero and rho >= 0"; return CE_E_BADARG; }
    const DevT &T = h->T;
    if (dy && (!A_vals_bm || !A_out_bm || (B > 1 && sA_b < T.nnz_aug))) { g_err = "ce_lpgd_perturb: dy needs A_vals_bm (batch-major rows at least nnz_aug apart) and A_out_bm"; return CE_E_BADARG; }
    const bool wP = P_out && nnz_p > 0 && rho != 0.0;
    const int rc = value_check_p(P_vals, p_rows, p_cols, wP ? nnz_p : 0, true);
    if (rc) return rc;
    CeLpgdPerturbArgs a{};
    a.B = B; a.n = T.n; a.m = T.m; a.nnz_aug = T.nnz_aug; a.nnz_p = wP ? nnz_p : 0;
    a.rowidx = h->d_rowidx.get(); a.colidx = h->d_colidx.get(); a.bpos = h->d_bpos.get(); a.prow = p_rows; a.pcol = p_cols;
    a.x = x; a.dx = dx; a.dy = dy; a.A = A_vals_bm; a.sAb = sA_b; a.q = q_vals; a.sqk = sq_k; a.sqb = sq_b; a.P = P_vals; a.tau = tau; a.rho = rho;
    a.q_out = q_out; a.A_out = dy ? A_out_bm : nullptr; a.P_out = wP ? P_out : nullptr; a.flags = flags;
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps(h, 2, st);
        ce_launch_lpgd_perturb(st, a);
    }
    HIPCHK(hipGetLastError());
    return CE_OK;
}
int ce_lpgd_grad(ce_handle h, int B, const double *x_a, const double *y_a, const double *x_b, const double *y_b, double delta, const unsigned char *skip,
                 double *dA_vals, long sdA_k, long sdA_b, double *dq_vals, long sdq_k, long sdq_b,
                 double *dP_vals, const int *p_rows, const int *p_cols, int nnz_p, void *stream) {
    if (!h || B <= 0 || !x_a || !y_a || !x_b || !y_b) { g_err = "null argument"; return CE_E_BADARG; }
    if (!(delta != 0.0)) { g_err = "ce_lpgd_grad: delta must be nonzero"; return CE_E_BADARG; }
    int rc = value_check_p(dP_vals, p_rows, p_cols, dP_vals ? nnz_p : 0, false);
    if (rc) return rc;
    const DevT &T = h->T;
    const int K = T.nnz_aug;
    const bool rows = dA_vals && sdA_k == 1 && (sdA_b >= K || B == 1), tile = dA_vals && !rows && sdA_b == 1 && sdA_k >= B;
    if (dA_vals && !rows && !tile) { g_err = "dA_vals must be batch-minor (sdA_k >= B, sdA_b = 1) or batch-major (sdA_k = 1, sdA_b >= nnz_aug)"; return CE_E_BADARG; }
    CeLpgdGradArgs a{};
    a.B = B; a.n = T.n; a.m = T.m; a.nnz_aug = K; a.nnz_p = dP_vals ? nnz_p : 0;
    a.rowidx = h->d_rowidx.get(); a.colidx = h->d_colidx.get(); a.prow = p_rows; a.pcol = p_cols;
    a.xa = x_a; a.ya = y_a; a.xb = x_b; a.yb = y_b; a.delta = delta; a.skip = skip;
    a.dA = dA_vals; a.sdAk = sdA_k; a.sdAb = sdA_b; a.dq = dq_vals; a.sdqk = sdq_k; a.sdqb = sdq_b; a.dP = dP_vals;
    const size_t lds_rows = ce_lpgd_grad_rows_lds(T.n, T.m), lds_tile = ce_lpgd_grad_tile_lds(T.n, T.m);
    if (lds_rows > VALUE_LDS_MAX) { g_err = "ce_lpgd_grad: the points of four instances exceed LDS"; return CE_E_TOO_LARGE; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    {
        ProfScope ps(h, 2, st);
        const bool tile_dq = tile && dq_vals && sdq_b == 1;      // (the tile kernel stores dq coalesced in that layout)
        if (tile) {
            // chunks of entries per tile.  Every chunk workgroup stages its tile's four vectors again, and a staged tile fills most of a CU's LDS (one workgroup
            // per CU at the metric shape): about one workgroup per CU and at least 1024 entries behind each staging pass (ce_value_vjp's rule -- 1024 workgroups,
            // at least 256 entries each -- staged four times as often here; DESIGN.md section 3.11 has both measurements)
            const int tiles = (B + 63) / 64;
            const int chunks = std::max(1, std::min((256 + tiles - 1) / tiles, (K + 1023) / 1024));
            const int kchunk = (K + chunks - 1) / chunks;
            ce_launch_lpgd_grad_tile(lds_tile <= VALUE_LDS_MAX, chunks, kchunk, tile_dq ? 1 : 0, lds_tile, st, a);
        }
        CeLpgdGradArgs r = a;
        if (tile) r.dA = nullptr;
        if (tile_dq) r.dq = nullptr;
        if (r.dA || r.dq || r.dP) ce_launch_lpgd_grad_rows(lds_rows, st, r);
    }
    HIPCHK(hipGetLastError());
    return CE_OK;
}

int ce_ca_step(ce_handle h, int B, int lp, double *W, double *UT, double *U, const double *PX, long ld_px, const double *QY, long ld_qy,
               const double *G, const double *PHI, const double *scale, const double *inv_den, const int *active,
               int update_w, int norm_after, double alpha, void *stream) {
    if (!h || B <= 0 || !W || !UT || !U || !PX || !QY || !G || !PHI || !scale || !inv_den || !active) { g_err = "null argument"; return CE_E_BADARG; }
    HIPCHK(hipSetDevice(h->device));
    const DevT &T = h->T;
    const size_t lds = ((size_t)(T.n + T.m + 1) + 2 * std::max(T.nq, 1) + NW * 8) * 8;
    if (lds > 64 * 1024) { g_err = "constant-A path: instance vectors do not fit LDS"; return CE_E_TOO_LARGE; }
    hipLaunchKernelGGL(k_ca_step, dim3(B), dim3(NT), lds, (hipStream_t)stream, T, lp, W, UT, U, PX, ld_px, QY, ld_qy, G, PHI, scale, inv_den, active, update_w, norm_after, alpha);
    HIPCHK(hipGetLastError());
    return CE_OK;
}
int ce_ca_check(ce_handle h, int B, int lp, int iter, const ce_settings *settings, double *W, const double *UT, const double *U,
                const double *AX, long ld_ax, const double *ATY, long ld_aty, const double *D, const double *E,
                const double *b_hat, const double *c_hat, const double *sigma, const double *nrm_b0, const double *nrm_c0,
                double *scale, double *sum_log, int *n_log, int *last_scale_iter, int *active, int *status, int *iters,
                double *resid, int *rescaled, void *stream) {
    if (!h || B <= 0 || !settings || !W || !UT || !U || !AX || !ATY || !D || !E || !b_hat || !c_hat || !sigma || !scale || !active || !status || !iters || !resid || !rescaled) { g_err = "null argument"; return CE_E_BADARG; }
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_ca_check, dim3(B), dim3(NT), NW * 8 * 8, (hipStream_t)stream, h->T, *settings, lp, iter, W, UT, U, AX, ld_ax, ATY, ld_aty, D, E, b_hat, c_hat,
                       sigma, nrm_b0, nrm_c0, scale, sum_log, n_log, last_scale_iter, active, status, iters, resid, rescaled);
    HIPCHK(hipGetLastError());
    return CE_OK;
}
int ce_ca_psd(ce_handle h, int B, int lp, double *U, const int *active, void *stream) {
    if (!h || B <= 0 || !U || !active) { g_err = "null argument"; return CE_E_BADARG; }
    if (h->T.ns == 0) return CE_OK;
    HIPCHK(hipSetDevice(h->device));
    const size_t lds = (2 * (size_t)h->T.maxs * h->T.maxs + 2 * h->T.maxs + 8 + NW * 8) * 8;
    if (lds > 64 * 1024) { g_err = "PSD order too large for the LDS-resident Jacobi projection"; return CE_E_TOO_LARGE; }
    hipLaunchKernelGGL(k_ca_psd, dim3(B, h->T.ns), dim3(NT), lds, (hipStream_t)stream, h->T, lp, U, active);
    HIPCHK(hipGetLastError());
    return CE_OK;
}
int ce_ca_psd_mfma(ce_handle h, int B, int lp, double *U, double *Vstate, int warm, const int *active, void *stream) {
    if (!h || B <= 0 || !U || !Vstate || !active) { g_err = "null argument"; return CE_E_BADARG; }
    if (h->T.ns == 0) return CE_OK;
    HIPCHK(hipSetDevice(h->device));
    const size_t lds = ((size_t)h->T.maxs * psd_refine_pitch(h->T.maxs) + psd_refine_scratch_doubles(h->T.maxs) + NW * 8) * 8;
    if (lds > 64 * 1024) { g_err = "PSD order too large for the LDS-resident MFMA projection (order <= 39)"; return CE_E_TOO_LARGE; }
    hipLaunchKernelGGL(k_ca_psd_mfma, dim3(B, h->T.ns), dim3(NT), lds, (hipStream_t)stream, h->T, lp, U, Vstate, warm, active);
    HIPCHK(hipGetLastError());
    return CE_OK;
}
int ce_solve_shared_a(ce_handle h, int B, int r, int RP, const double *AdT, const int *drow, const int *srow_col, const double *srow_val,
                      const int *scol_ptr, const int *scol_row, const double *gs, const double *Dv, const double *Ev, const double *b_hat,
                      const double *c_hat, const double *sigma, const double *nrm_b0, const double *nrm_c0, const ce_settings *settings,
                      const double *warm_x, const double *warm_y, const double *warm_s,
                      double *x, double *y, double *s, int *iters, int *status, double *resid, void *stream) {
    if (!h || B <= 0 || !AdT || !drow || !srow_col || !srow_val || !scol_ptr || !scol_row || !gs || !Dv || !Ev || !b_hat || !c_hat || !sigma || !nrm_b0 || !nrm_c0 ||
        !settings || !x || !y || !s || !iters || !status) { g_err = "null argument"; return CE_E_BADARG; }
    const DevT &T = h->T;
    if (r < 0 || r > RP || (RP != 16 && RP != 32 && RP != 64)) { g_err = "shared-A forward kernel: at most 64 dense rows (RP in 16, 32, 64)"; return CE_E_UNSUPPORTED; }
    const SaFwdSel sel = sa_fwd_select(T, r, RP, settings->acceleration_lookback > 0);
    if (sel.lds == 0) { g_err = "shared-A forward kernel: the iterates of one instance do not fit LDS"; return CE_E_TOO_LARGE; }
    HIPCHK(hipSetDevice(h->device));
    if (!h->sa_fwd_attr) { HIPCHK(ce_setattr_sa_fwd((int)LDS_LIMIT)); h->sa_fwd_attr = true; }
    if (!h->d_psd_stats.get() && T.ns > 0) {
        const char *e = getenv("CE_PSD_STATS");
        if (e && atoi(e) != 0) { HIPCHK(h->d_psd_stats.reserve(16)); HIPCHK(hipMemset(h->d_psd_stats.get(), 0, 16 * sizeof(unsigned long long))); }
    }
    int psd_refine = 1; if (const char *e = getenv("CE_PSD_REFINE")) psd_refine = atoi(e) != 0;
    double *aa_ws = nullptr;
    if (settings->acceleration_lookback > 0) {
        const size_t l = (size_t)T.n + T.m + 1, lp = l + (l & 1);
        HIPCHK(h->d_aa_ws.reserve((size_t)B * 4 * lp));
        aa_ws = h->d_aa_ws.get();
    }
    const CeSaFwdArgs fa{T, SaFwd{r, RP, AdT, drow, srow_col, srow_val, scol_ptr, scol_row, gs, Dv, Ev, h->d_psd_stats.get(), aa_ws, sel.aa_w_lds, psd_refine}, *settings,
                         b_hat, c_hat, sigma, nrm_b0, nrm_c0, warm_x, warm_y, warm_s, x, y, s, iters, status, resid};
    {
        ProfScope ps(h, 0, (hipStream_t)stream);
        if (ce_launch_sa_fwd(sel.row, B, sel.lds, (hipStream_t)stream, fa)) { g_err = "internal: no shared-A forward kernel for the selected variant"; return CE_E_BADARG; }
        h->last_sa_fwd = sel.row;
    }
    HIPCHK(hipGetLastError());
    return CE_OK;
}
static int vjp_lsqr_launch(ce_handle h, int B, const double *A_vals0, long sA_b, int per_inst, const double *q_vals, long sq_k, long sq_b,
                           const double *x, const double *y, const double *s, const double *dx, const double *dy,
                           double *dA_bm, double *dq_vals, long sdq_k, long sdq_b, int *adj_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream,
                           const int *sel, int status_or, int *sel_reset, const SaJvp *fwd, const SaWalkMany *many) {
    // fwd != nullptr: the forward derivative (ce_jvp_lsqr / ce_jvp_shared_a) -- k_sa_lsqr<..., FWD> on the same plan; dx ... dq_vals are unused
    // many != nullptr (with sel): the list is walked for many->K right-hand sides in this ONE launch; the pointers are those of right-hand side 0
    if (!h || B <= 0 || !A_vals0 || !x || !y || !s) { g_err = "null argument"; return CE_E_BADARG; }
    if (fwd ? (!fwd->dx || !fwd->dy) : (!dx || !dy || !dA_bm || !dq_vals)) { g_err = "null argument"; return CE_E_BADARG; }
    const DevT &T = h->T;
    const SaLsqrSel sl = sa_lsqr_select(T, h->sp_RP, h->psd_first, h->lsqr_variant, per_inst != 0, sel != nullptr, fwd != nullptr);
    if (sl.lds == 0) { g_err = fwd ? "forward-derivative kernel: the LSQR vectors of one instance do not fit LDS" : "shared-A adjoint kernel: the LSQR vectors of one instance do not fit LDS"; return CE_E_TOO_LARGE; }
    const int RP = sl.RP;
    HIPCHK(hipSetDevice(h->device));
    if (!h->sa_lsqr_attr) { HIPCHK(ce_setattr_sa_lsqr((int)LDS_LIMIT)); h->sa_lsqr_attr = true; }
    // The streaming passes read c_j of their instance with every row of the matrix.  In the boundary's layout (q_eval (n + 1, B): consecutive j are B doubles apart) each of
    // those loads is a line of its own, and the lines of all resident instances (config 5: 768 x 501 x 128 B) live in the memory-side cache, not in L2: the pass waited for
    // THEM, not for the matrix.  One transpose per call gives every instance a contiguous c (4 KB, L2-resident for the whole solve).  Not for the re-solve list
    // (a handful of instances; the launch sits on the metric configuration's hot path).
    if (q_vals && !sel && sq_b == 1 && sq_k == (long)B && B > 1) {
        HIPCHK(h->d_qT.reserve((size_t)B * (T.n + 1)));
        launch_transpose((hipStream_t)stream, q_vals, h->d_qT.get(), T.n + 1, B);
        q_vals = h->d_qT.get(); sq_k = 1; sq_b = T.n + 1;
    }
    const CeSaLsqrArgs la{T, SaStruct{h->d_csc_ptr.get(), h->d_rowidx.get(), h->d_csr_ptr.get(), h->d_csr_col.get(), h->d_csr_src.get(), T.nnzA, h->d_bpos.get()},
                          SaSplit{h->sp_r, RP, h->d_sp_AdT.get(), h->d_sp_drow.get(), h->d_sp_srow_col.get(), h->d_sp_sval.get(), h->d_sp_scol_ptr.get(), h->d_sp_scol_row.get(),
                                  h->d_sp_rowslot.get(), h->d_sp_sing_i.get(), h->d_sp_sing_v.get()},
                          A_vals0, sA_b, per_inst, q_vals, sq_k, sq_b, x, y, s, dx, dy, dA_bm, dq_vals, sdq_k, sdq_b, adj_status, lsqr_iters,
                          atol, btol, conlim, iter_lim > 0 ? iter_lim : 2 * (T.n + T.m + 1), sel, status_or, sl.a_lds, sel_reset, fwd ? *fwd : SaJvp{}, (many && sel) ? *many : SaWalkMany{}};
    if (RP > 0) {      // the values may differ between calls: refill A_d^T / singleton values from this call's A (n RP + m doubles)
        HIPCHK(hipMemsetAsync(h->d_sp_AdT.get(), 0, sizeof(double) * (size_t)T.n * RP, (hipStream_t)stream));
        HIPCHK(hipMemsetAsync(h->d_sp_sval.get(), 0, sizeof(double) * T.m, (hipStream_t)stream));
        HIPCHK(hipMemsetAsync(h->d_sp_sing_v.get(), 0, sizeof(double) * T.n, (hipStream_t)stream));
        if (T.nnzA > 0) ce_launch_sa_fill_split((hipStream_t)stream, T.nnzA, RP, h->d_rowidx.get(), h->d_colidx.get(), h->d_sp_rowslot.get(), A_vals0,
                                                h->d_sp_AdT.get(), h->d_sp_sval.get(), h->d_sp_sing_i.get(), h->d_sp_sing_v.get());
    }
    {
        ProfScope ps(h, 1, (hipStream_t)stream);
        if (ce_launch_sa_lsqr(sl.row, B, sl.lds, (hipStream_t)stream, la)) { g_err = "internal: no LSQR kernel for the selected variant"; return CE_E_BADARG; }
        h->last_sa_lsqr = sl.row;
    }
    HIPCHK(hipGetLastError());
    return CE_OK;
}
int ce_vjp_shared_a(ce_handle h, int B, const double *A_vals0, long sA_b, const double *q_vals, long sq_k, long sq_b,
                    const double *x, const double *y, const double *s, const double *dx, const double *dy,
                    double *dA_bm, double *dq_vals, long sdq_k, long sdq_b, int *adj_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream) {
    return vjp_lsqr_launch(h, B, A_vals0, sA_b, 0, q_vals, sq_k, sq_b, x, y, s, dx, dy, dA_bm, dq_vals, sdq_k, sdq_b, adj_status, lsqr_iters, atol, btol, conlim, iter_lim, stream);
}
int ce_vjp_lsqr(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                const double *x, const double *y, const double *s, const double *dx, const double *dy,
                double *dA_bm, double *dq_vals, long sdq_k, long sdq_b, int *adj_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream) {
    if (sA_b == 0 && B > 1) { g_err = "ce_vjp_lsqr: per-instance values need a batch stride"; return CE_E_BADARG; }
    return vjp_lsqr_launch(h, B, A_vals_bm, sA_b, 1, q_vals, sq_k, sq_b, x, y, s, dx, dy, dA_bm, dq_vals, sdq_k, sdq_b, adj_status, lsqr_iters, atol, btol, conlim, iter_lim, stream);
}
static int jvp_lsqr_launch(ce_handle h, int B, const double *A_vals0, long sA_b, int per_inst, const double *q_vals, long sq_k, long sq_b,
                           const double *x, const double *y, const double *s, const double *tA_vals_bm, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                           double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream,
                           const int *sel = nullptr, int status_or = 0, int *sel_reset = nullptr, const SaWalkMany *many = nullptr) {
    // sel: the re-solve list of ce_jvp (B is then the fixed grid that walks it; the kernel addresses every per-instance array by the LISTED instance)
    if (!h) { g_err = "null argument"; return CE_E_BADARG; }
    if (h->plan.qp_native) { g_err = "forward derivative: not available with a quadratic objective inside the kernels; use the epigraph form (cone form) of the problem"; return CE_E_UNSUPPORTED; }
    const SaJvp W{tA_vals_bm, stA_b, tq_vals, stq_k, stq_b, dx, dy, ds};
    return vjp_lsqr_launch(h, B, A_vals0, sA_b, per_inst, q_vals, sq_k, sq_b, x, y, s, nullptr, nullptr, nullptr, nullptr, 0, 0, jvp_status, lsqr_iters, atol, btol, conlim, iter_lim, stream,
                           sel, status_or, sel_reset, &W, many);
}
int ce_jvp_shared_a(ce_handle h, int B, const double *A_vals0, long sA_b, const double *q_vals, long sq_k, long sq_b,
                    const double *x, const double *y, const double *s, const double *tA_vals_bm, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                    double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream) {
    return jvp_lsqr_launch(h, B, A_vals0, sA_b, 0, q_vals, sq_k, sq_b, x, y, s, tA_vals_bm, stA_b, tq_vals, stq_k, stq_b, dx, dy, ds, jvp_status, lsqr_iters, atol, btol, conlim, iter_lim, stream);
}
int ce_jvp_lsqr(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                const double *x, const double *y, const double *s, const double *tA_vals_bm, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream) {
    if (sA_b == 0 && B > 1) { g_err = "ce_jvp_lsqr: per-instance values need a batch stride"; return CE_E_BADARG; }
    return jvp_lsqr_launch(h, B, A_vals_bm, sA_b, 1, q_vals, sq_k, sq_b, x, y, s, tA_vals_bm, stA_b, tq_vals, stq_k, stq_b, dx, dy, ds, jvp_status, lsqr_iters, atol, btol, conlim, iter_lim, stream);
}
// a call that runs the elimination with a quadratic objective inside (`who`): the template must have planned one
static int qp_ns_check(ce_handle h, const char *who) {
    if (!h->plan.qp_native) { g_err = std::string(who) + ": this template does not run a quadratic objective inside the kernels (ce_qp_native == 0)"; return CE_E_UNSUPPORTED; }
    if (h->plan.qp_ns_variant < 0) { g_err = std::string(who) + ": this template has no search-free elimination with a quadratic objective (n > 108, its footprint exceeds LDS, or CE_BWD_NS=0)"; return CE_E_UNSUPPORTED; }
    return CE_OK;
}
// The forward derivative as ce_vjp_qp runs the adjoint: the search-free elimination (k_backward_ns<..., FWD>), then the fixed grid of LSQR workgroups that
// re-solves the instances it listed as rank deficient -- the same re-solve list.  With P_vals (ce_jvp_qp: k_backward_ns<..., FWD, QP>) one launch and no re-solve list: no LSQR has a P term.
static int jvp_ns(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b, const double *P_vals,
                  const double *x, const double *y, const double *s, const double *tA_vals_bm, long stA_b, const double *tq_vals, long stq_k, long stq_b, const double *tP_vals,
                  double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream, bool psd = false, bool psd_tri = false) {          // (psd_tri: ce_jvp_psd_tri -- PSD blocks and triples, the row with both kinds' segments)
    const bool qp = P_vals != nullptr;
    const std::string who = qp ? "ce_jvp_qp" : (psd_tri ? "ce_jvp_psd_tri" : (psd ? "ce_jvp_psd" : "ce_jvp"));
    const CePlan &P = h->plan;
    const DevT &T = h->T;
    int rc = CE_OK;
    if (qp) { rc = qp_ns_check(h, "ce_jvp_qp"); if (rc) return rc; }
    else if (psd_tri) {  // (the opt-in entry point of templates with PSD blocks and triples: ce_jvp and ce_jvp_psd keep refusing them)
        if (P.psd_tri_ns_variant < 0) { g_err = "ce_jvp_psd_tri: this template has no search-free elimination with PSD blocks and triples (it lacks a PSD block or an exponential / power cone, has a quadratic objective, n > 108, its footprint exceeds LDS, or CE_BWD_NS=0); use ce_jvp_lsqr"; return CE_E_UNSUPPORTED; }
    } else if (psd) {      // (the opt-in entry point of PSD templates: ce_jvp itself keeps refusing them)
        if (P.psd_ns_variant < 0) { g_err = "ce_jvp_psd: this template has no search-free elimination with PSD blocks (no PSD block, triples or a quadratic objective beside them, n > 108, its footprint exceeds LDS, or CE_BWD_NS=0); use ce_jvp_lsqr"; return CE_E_UNSUPPORTED; }
    } else {
        if (P.qp_native) { g_err = "forward derivative: not available with a quadratic objective inside the kernels; use the epigraph form (cone form) of the problem"; return CE_E_UNSUPPORTED; }
        if (P.ns_variant < 0 && P.tri_ns_variant < 0) { g_err = "ce_jvp: this template has no search-free elimination (PSD / exponential / power cones, or n > 108); use ce_jvp_lsqr"; return CE_E_UNSUPPORTED; }
        if (!resolve_fits(h)) { g_err = "ce_jvp: the LSQR vectors of the re-solve exceed LDS; use ce_jvp_lsqr"; return CE_E_UNSUPPORTED; }
    }
    const bool tri = !qp && !psd && !psd_tri && P.ns_variant < 0;      // exponential / power triples: k_backward_ns<..., FWD, TRI> on its own footprint, the same re-solve list behind it
    const int variant = qp ? P.qp_ns_variant : (psd_tri ? P.psd_tri_ns_variant : (psd ? P.psd_ns_variant : (tri ? P.tri_ns_variant : P.ns_variant)));
    const size_t lds = qp ? P.qp_ns_lds : (psd_tri ? P.psd_tri_ns_lds : (psd ? P.psd_ns_lds : (tri ? P.tri_ns_lds : P.ns_lds)));
    if (B > 1 && (sA_b != T.nnz_aug || (tA_vals_bm && stA_b != T.nnz_aug))) { g_err = who + ": A_vals_bm and tA_vals_bm must be contiguous batch-major rows"; return CE_E_BADARG; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    FixLists fix{nullptr, nullptr};
    if (!qp) { rc = resolve_lists(h, B, st, &fix); if (rc) return rc; }
    ProfScope ps(h, 1, st);
    CeBwdArgs ba{};
    ba.T = T; ba.T.lda = T.n; ba.Abm = A_vals_bm; ba.x = x; ba.y = y; ba.s = s; ba.adj = jvp_status; ba.fix = fix.cur;
    const NsJvp W{h->d_csc_ptr.get(), h->d_csr_ptr.get(), h->d_csr_col.get(), h->d_csr_src.get(), h->d_bpos.get(), tA_vals_bm, tq_vals, stq_k, stq_b, dx, dy, ds, lsqr_iters};
    const int lrc = qp ? ce_launch_ns(variant, B, lds, st, ba, NsJvpQp{W, NsQp{P_vals, tP_vals, h->d_pmap.get(), h->nnz_p}})
                  : psd_tri ? ce_launch_ns(variant, B, lds, st, ba, NsJvpPsdTri{W})
                  : psd ? ce_launch_ns(variant, B, lds, st, ba, NsJvpPsd{W})
                  : tri ? ce_launch_ns(variant, B, lds, st, ba, NsJvpTri{W}) : ce_launch_ns(variant, B, lds, st, ba, W);
    if (lrc) { g_err = "internal: no forward elimination kernel for the planned variant"; return CE_E_BADARG; }
    if (!qp) {
        rc = resolve_run(h, B, fix, [&](int grid, const int *sel, int status_or, int *sel_reset) {
            return jvp_lsqr_launch(h, grid, A_vals_bm, sA_b, 1, q_vals, sq_k, sq_b, x, y, s, tA_vals_bm, stA_b, tq_vals, stq_k, stq_b, dx, dy, ds, jvp_status, lsqr_iters,
                                   atol, btol, conlim, iter_lim, stream, sel, status_or, sel_reset);
        });
        if (rc) return rc;
    }
    HIPCHK(hipGetLastError());
    return CE_OK;
}
int ce_jvp(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
           const double *x, const double *y, const double *s, const double *tA_vals_bm, long stA_b, const double *tq_vals, long stq_k, long stq_b,
           double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream) {
    if (!h || B <= 0 || !A_vals_bm || !x || !y || !s || !dx || !dy || !jvp_status) { g_err = "null argument"; return CE_E_BADARG; }
    return jvp_ns(h, B, A_vals_bm, sA_b, q_vals, sq_k, sq_b, nullptr, x, y, s, tA_vals_bm, stA_b, tq_vals, stq_k, stq_b, nullptr, dx, dy, ds, jvp_status, lsqr_iters, atol, btol, conlim, iter_lim, stream);
}
int ce_jvp_psd(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
               const double *x, const double *y, const double *s, const double *tA_vals_bm, long stA_b, const double *tq_vals, long stq_k, long stq_b,
               double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream) {
    if (!h || B <= 0 || !A_vals_bm || !x || !y || !s || !dx || !dy || !jvp_status) { g_err = "null argument"; return CE_E_BADARG; }
    return jvp_ns(h, B, A_vals_bm, sA_b, q_vals, sq_k, sq_b, nullptr, x, y, s, tA_vals_bm, stA_b, tq_vals, stq_k, stq_b, nullptr, dx, dy, ds, jvp_status, lsqr_iters, atol, btol, conlim, iter_lim, stream, true);
}
int ce_jvp_psd_tri(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                   const double *x, const double *y, const double *s, const double *tA_vals_bm, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                   double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream) {
    if (!h || B <= 0 || !A_vals_bm || !x || !y || !s || !dx || !dy || !jvp_status) { g_err = "ce_jvp_psd_tri: null argument"; return CE_E_BADARG; }
    return jvp_ns(h, B, A_vals_bm, sA_b, q_vals, sq_k, sq_b, nullptr, x, y, s, tA_vals_bm, stA_b, tq_vals, stq_k, stq_b, nullptr, dx, dy, ds, jvp_status, lsqr_iters, atol, btol, conlim, iter_lim, stream, false, true);
}
int ce_jvp_qp(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *P_vals, const double *x, const double *y, const double *s,
              const double *tA_vals_bm, long stA_b, const double *tq_vals, long stq_k, long stq_b, const double *tP_vals,
              double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, void *stream) {
    if (!h || B <= 0 || !A_vals_bm || !P_vals || !x || !y || !s || !dx || !dy || !jvp_status) { g_err = "null argument"; return CE_E_BADARG; }
    return jvp_ns(h, B, A_vals_bm, sA_b, nullptr, 0, 0, P_vals, x, y, s, tA_vals_bm, stA_b, tq_vals, stq_k, stq_b, tP_vals, dx, dy, ds, jvp_status, lsqr_iters, 0.0, 0.0, 0.0, 0, stream);
}
// K tangents at one solution (include/cone_engine.h).  One launch of k_backward_ns<..., FWD, ..., MANY> factors every instance once and writes all K answers; plain kind:
// the instances it lists as rank deficient are listed ONCE, and ONE launch of the LSQR kernel walks the K x list (tangent, instance) pairs (SaWalkMany; the list parity
// flips once).  QP kind: no re-solve, the dropped-variable answer stands with status 4 for every k.  tri: ce_jvp_tri_many -- the plain kind's body with
// k_backward_ns<..., FWD, ..., TRI, MANY> on the triples' variant and footprint; psd: ce_jvp_psd_many -- with k_backward_ns<..., FWD, ..., MANY, PSD> on the blocks'.
static int jvp_many_ns(ce_handle h, NsManyKind kind, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b, const double *P_vals,
                       const double *x, const double *y, const double *s, const double *tA_vals, long stA_k, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                       const double *tP_vals, long stP_k, long stP_b, double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters,
                       double atol, double btol, double conlim, int iter_lim, void *stream) {
    const bool qp = P_vals != nullptr, tri = kind == NS_MANY_TRI, psd = kind == NS_MANY_PSD, psd_tri = kind == NS_MANY_PSD_TRI;
    const std::string who = qp ? "ce_jvp_qp_many" : (psd_tri ? "ce_jvp_psd_tri_many" : (psd ? "ce_jvp_psd_many" : (tri ? "ce_jvp_tri_many" : "ce_jvp_many")));
    const CePlan &P = h->plan;
    const DevT &T = h->T;
    if (qp) { const int rc = qp_ns_check(h, "ce_jvp_qp_many"); if (rc) return rc; }
    if ((qp ? ce_jvp_qp_many_variant(h) : psd_tri ? ce_jvp_psd_tri_many_variant(h) : (psd ? ce_jvp_psd_many_variant(h) : (tri ? ce_jvp_tri_many_variant(h) : ce_jvp_many_variant(h)))) < 0) {
        g_err = who + (qp ? ": this template has no many-tangent elimination with a quadratic objective; call ce_jvp_qp once per tangent"
                       : psd_tri ? ": this template has no search-free elimination with PSD blocks and triples (it lacks a PSD block or an exponential / power cone, has a quadratic objective, n > 108, its footprint exceeds LDS, or CE_BWD_NS=0); call ce_jvp_lsqr once per tangent"
                       : psd ? ": this template has no search-free elimination with PSD blocks (no PSD block, triples or a quadratic objective beside them, n > 108, its "
                               "footprint exceeds LDS, or CE_BWD_NS=0); call ce_jvp_lsqr once per tangent"
                       : tri ? ": this template has no search-free elimination with triples (no exponential / power cone, PSD cones, a quadratic objective inside the "
                               "kernels, n > 108, CE_BWD_NS=0, or the LSQR vectors of the re-solve exceed LDS); call ce_jvp_many or ce_jvp"
                          : ": this template has no many-tangent elimination (PSD / exponential / power cones, a quadratic objective inside the kernels, n > 108, CE_BWD_NS=0, "
                            "or the LSQR vectors of the re-solve exceed LDS); call ce_jvp once per tangent");
        return CE_E_UNSUPPORTED;
    }
    const long nnz = T.nnz_aug, n = T.n, m = T.m;
    if (B > 1 && sA_b != nnz) { g_err = who + ": A_vals_bm must be contiguous batch-major rows"; return CE_E_BADARG; }
    if ((tA_vals && stA_b != 0 && stA_b < nnz) || (tq_vals && stq_b != 0 && stq_b < n + 1) || (tP_vals && stP_b != 0 && stP_b < (long)h->nnz_p)) {
        g_err = who + ": a tangent's batch stride is 0 (one row shared by the batch) or at least the row length"; return CE_E_BADARG;
    }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    FixLists fix{nullptr, nullptr};
    int rc = CE_OK;
    if (!qp) { rc = resolve_lists(h, B, st, &fix); if (rc) return rc; }
    ProfScope ps(h, 1, st);
    CeBwdArgs ba{};
    ba.T = T; ba.T.lda = T.n; ba.Abm = A_vals_bm; ba.x = x; ba.y = y; ba.s = s; ba.adj = jvp_status; ba.fix = fix.cur;
    const long sxk = (long)((size_t)B * n), syk = (long)((size_t)B * m), sak = B;
    const NsJvpMany W{h->d_csc_ptr.get(), h->d_csr_ptr.get(), h->d_csr_col.get(), h->d_csr_src.get(), h->d_bpos.get(), K, tA_vals, stA_k, stA_b, tq_vals, stq_k, stq_b,
                      dx, dy, ds, sxk, syk, sak, lsqr_iters};
    const int lrc = qp ? ce_launch_ns(P.qp_ns_variant, B, P.qp_ns_lds, st, ba, NsJvpQpMany{W, NsQp{P_vals, tP_vals, h->d_pmap.get(), h->nnz_p}, stP_k, stP_b})
                       : psd_tri ? ce_launch_ns(P.psd_tri_ns_variant, B, P.psd_tri_ns_lds, st, ba, NsJvpManyPsdTri{W})
                       : psd ? ce_launch_ns(P.psd_ns_variant, B, P.psd_ns_lds, st, ba, NsJvpManyPsd{W})
                       : tri ? ce_launch_ns(P.tri_ns_variant, B, P.tri_ns_lds, st, ba, NsJvpManyTri{W}) : ce_launch_ns(P.ns_variant, B, P.ns_lds, st, ba, W);
    if (lrc) { g_err = "internal: no many-tangent kernel for the planned variant"; return CE_E_BADARG; }
    if (!qp) {
        const int grid = B < 768 ? B : 768;          // (resolve_run's grid)
        const int prof_keep = h->prof; h->prof = 0;
        SaWalkMany wm; wm.K = K; wm.stAk = stA_k; wm.stqk = stq_k; wm.sok = sxk; wm.sosk = syk; wm.sak = sak;
        rc = jvp_lsqr_launch(h, grid, A_vals_bm, sA_b, 1, q_vals, sq_k, sq_b, x, y, s, tA_vals, stA_b, tq_vals, 1, stq_b, dx, dy, ds, jvp_status, lsqr_iters,
                             atol, btol, conlim, iter_lim, stream, fix.cur, 4 | 8, fix.oth, &wm);
        h->fix_par ^= 1;
        h->prof = prof_keep;
        if (rc) return rc;
    }
    HIPCHK(hipGetLastError());
    return CE_OK;
}
int ce_jvp_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                const double *x, const double *y, const double *s, const double *tA_vals, long stA_k, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream) {
    if (!h || B <= 0 || K <= 0 || !A_vals_bm || !x || !y || !s || !dx || !dy || !jvp_status || stA_b < 0 || stq_b < 0) {
        g_err = "ce_jvp_many: null argument, B <= 0, K <= 0 or a negative batch stride"; return CE_E_BADARG;
    }
    if (h->plan.qp_native) { g_err = "ce_jvp_many: this template runs a quadratic objective inside the kernels; use ce_jvp_qp_many"; return CE_E_UNSUPPORTED; }
    return jvp_many_ns(h, NS_MANY_PLAIN, B, K, A_vals_bm, sA_b, q_vals, sq_k, sq_b, nullptr, x, y, s, tA_vals, stA_k, stA_b, tq_vals, stq_k, stq_b, nullptr, 0, 0, dx, dy, ds, jvp_status, lsqr_iters,
                       atol, btol, conlim, iter_lim, stream);
}
// K tangents at one solution of a template with exponential / power triples (include/cone_engine.h): ce_jvp_many's body with k_backward_ns<..., FWD, ..., TRI, MANY> on
// the triples' variant and footprint; the re-solve behind it is the same one launch.  Refusals come before any device call.
int ce_jvp_tri_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                    const double *x, const double *y, const double *s, const double *tA_vals, long stA_k, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                    double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream) {
    if (!h || B <= 0 || K <= 0 || !A_vals_bm || !x || !y || !s || !dx || !dy || !jvp_status || stA_b < 0 || stq_b < 0) {
        g_err = "ce_jvp_tri_many: null argument, B <= 0, K <= 0 or a negative batch stride"; return CE_E_BADARG;
    }
    return jvp_many_ns(h, NS_MANY_TRI, B, K, A_vals_bm, sA_b, q_vals, sq_k, sq_b, nullptr, x, y, s, tA_vals, stA_k, stA_b, tq_vals, stq_k, stq_b, nullptr, 0, 0, dx, dy, ds, jvp_status, lsqr_iters,
                       atol, btol, conlim, iter_lim, stream);
}
// K tangents at one solution of a template with PSD blocks (include/cone_engine.h): ce_jvp_many's body with k_backward_ns<..., FWD, ..., MANY, PSD> on the blocks'
// variant and footprint; the re-solve behind it is the same one launch.  Refusals come before any device call.
int ce_jvp_psd_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                    const double *x, const double *y, const double *s, const double *tA_vals, long stA_k, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                    double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream) {
    if (!h || B <= 0 || K <= 0 || !A_vals_bm || !x || !y || !s || !dx || !dy || !jvp_status || stA_b < 0 || stq_b < 0) {
        g_err = "ce_jvp_psd_many: null argument, B <= 0, K <= 0 or a negative batch stride"; return CE_E_BADARG;
    }
    return jvp_many_ns(h, NS_MANY_PSD, B, K, A_vals_bm, sA_b, q_vals, sq_k, sq_b, nullptr, x, y, s, tA_vals, stA_k, stA_b, tq_vals, stq_k, stq_b, nullptr, 0, 0, dx, dy, ds, jvp_status, lsqr_iters,
                       atol, btol, conlim, iter_lim, stream);
}
// K tangents at one solution of a template with PSD blocks AND triples (include/cone_engine.h): ce_jvp_many's body with k_backward_ns<..., FWD, ..., TRI, MANY, PSD> on
// the variant and footprint with both kinds' segments; the re-solve behind it is the same one launch.  Refusals come before any device call.
int ce_jvp_psd_tri_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b,
                        const double *x, const double *y, const double *s, const double *tA_vals, long stA_k, long stA_b, const double *tq_vals, long stq_k, long stq_b,
                        double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, double atol, double btol, double conlim, int iter_lim, void *stream) {
    if (!h || B <= 0 || K <= 0 || !A_vals_bm || !x || !y || !s || !dx || !dy || !jvp_status || stA_b < 0 || stq_b < 0) {
        g_err = "ce_jvp_psd_tri_many: null argument, B <= 0, K <= 0 or a negative batch stride"; return CE_E_BADARG;
    }
    return jvp_many_ns(h, NS_MANY_PSD_TRI, B, K, A_vals_bm, sA_b, q_vals, sq_k, sq_b, nullptr, x, y, s, tA_vals, stA_k, stA_b, tq_vals, stq_k, stq_b, nullptr, 0, 0, dx, dy, ds, jvp_status, lsqr_iters,
                       atol, btol, conlim, iter_lim, stream);
}
int ce_jvp_qp_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *P_vals, const double *x, const double *y, const double *s,
                   const double *tA_vals, long stA_k, long stA_b, const double *tq_vals, long stq_k, long stq_b, const double *tP_vals, long stP_k, long stP_b,
                   double *dx, double *dy, double *ds, int *jvp_status, int *lsqr_iters, void *stream) {
    if (!h || B <= 0 || K <= 0 || !A_vals_bm || !P_vals || !x || !y || !s || !dx || !dy || !jvp_status || stA_b < 0 || stq_b < 0 || stP_b < 0) {
        g_err = "ce_jvp_qp_many: null argument, B <= 0, K <= 0 or a negative batch stride"; return CE_E_BADARG;
    }
    return jvp_many_ns(h, NS_MANY_PLAIN, B, K, A_vals_bm, sA_b, nullptr, 0, 0, P_vals, x, y, s, tA_vals, stA_k, stA_b, tq_vals, stq_k, stq_b, tP_vals, stP_k, stP_b, dx, dy, ds, jvp_status, lsqr_iters,
                       0.0, 0.0, 0.0, 0, stream);
}
// K cotangents at one solution of a template with a quadratic objective inside the kernels (include/cone_engine.h).  One launch of k_backward_ns<..., QP, ..., MANY>
// without FWD factors every instance once and writes all K answers, dP among them.  No re-solve list: no LSQR has a P term, the dropped-variable answer of a
// rank-deficient instance stands with status 4 for every k (as ce_jvp_qp_many and ce_vjp_qp).
// (rec: ce_vjp_qp_many_params -- the kernel stores the pairs' factor records [K][B][rpitch] and neither dA rows nor dP; dA_vals and dP_vals are unused then)
static int vjp_qp_many_run(ce_handle h, const char *who, int B, int K, const double *A_vals_bm, long sA_b, const double *P_vals, const double *x, const double *y, const double *s,
                           const double *dx, const double *dy, double *dA_vals, double *dq_vals, double *dP_vals, int *adj_status, void *stream, double *rec = nullptr, long rpitch = 0) {
    const CePlan &P = h->plan;
    const DevT &T = h->T;
    if (B > 1 && sA_b != T.nnz_aug) { g_err = std::string(who) + ": A_vals_bm must be contiguous batch-major rows"; return CE_E_BADARG; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t n = T.n, m = T.m, nnz = T.nnz_aug, nnzp = (size_t)h->nnz_p;
    long syk = (long)((size_t)B * m);
    if (!dy) {
        HIPCHK(h->d_dy0.reserve((size_t)B * m));
        HIPCHK(hipMemsetAsync(h->d_dy0.get(), 0, sizeof(double) * (size_t)B * m, st));
        dy = h->d_dy0.get(); syk = 0;
    }
    NsVjpQpMany W{};
    W.K = K; W.sxk = (long)((size_t)B * n); W.syk = syk; W.sAk = (long)((size_t)B * nnz); W.sqk = (long)((size_t)B * (n + 1)); W.sak = (long)B;
    W.Q = NsQp{P_vals, nullptr, h->d_pmap.get(), h->nnz_p};
    W.prow = h->d_prow.get(); W.pcol = h->d_pcol.get(); W.p_tri = h->p_tri; W.dP = dP_vals; W.sPk = (long)((size_t)B * nnzp);
    if (rec) { W.rec = rec; W.rpitch = rpitch; W.srk = (long)((size_t)B * rpitch); W.dP = nullptr; dA_vals = nullptr; }          // (record mode writes through neither)
    ProfScope ps(h, 1, st);
    CeBwdArgs ba{};
    ba.T = T; ba.T.lda = T.n; ba.Abm = A_vals_bm; ba.x = x; ba.y = y; ba.s = s; ba.dx = dx; ba.dy = dy; ba.dA = dA_vals; ba.dq = dq_vals; ba.sdqk = 1; ba.sdqb = (long)(n + 1);
    ba.adj = adj_status; ba.fix = nullptr;
    h->last_fast = -1;
    if (ce_launch_ns(P.qp_ns_variant, B, P.qp_ns_lds, st, ba, W)) { g_err = "internal: no many-cotangent kernel with a quadratic objective for the planned variant"; return CE_E_BADARG; }
    HIPCHK(hipGetLastError());
    return CE_OK;
}
int ce_vjp_qp_many(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *P_vals, const double *x, const double *y, const double *s,
                   const double *dx, const double *dy, double *dA_vals, double *dq_vals, double *dP_vals, int *adj_status, void *stream) {
    if (!h || B <= 0 || K <= 0 || !A_vals_bm || !P_vals || !x || !y || !s || !dx || !dA_vals || !dq_vals || !dP_vals) {
        g_err = "ce_vjp_qp_many: null argument, B <= 0 or K <= 0"; return CE_E_BADARG;
    }
    { const int rc = qp_ns_check(h, "ce_vjp_qp_many"); if (rc) return rc; }
    return vjp_qp_many_run(h, "ce_vjp_qp_many", B, K, A_vals_bm, sA_b, P_vals, x, y, s, dx, dy, dA_vals, dq_vals, dP_vals, adj_status, stream);
}
// The parameter gradients of K cotangents of a native QP, neither dA nor dP in memory (include/cone_engine.h): ce_vjp_qp_many's one launch in record mode and
// k_param_grad behind it, whose map carries P entries beside the A and q entries.  No re-solve: a rank-deficient instance keeps the dropped-variable answer, status 4.
int ce_vjp_qp_many_params(ce_handle h, int B, int K, const double *A_vals_bm, long sA_b, const double *P_vals, const double *x, const double *y, const double *s,
                          const double *dx, const double *dy, int rows, const int *map_ptr, const int *map_code, const int *map_k, const double *map_val,
                          double *g, double *dq_vals, int *adj_status, void *stream) {
    if (!h || B <= 0 || K <= 0 || !A_vals_bm || !P_vals || !x || !y || !s || !dx || !g || !dq_vals || !adj_status) {
        g_err = "ce_vjp_qp_many_params: null argument, B <= 0 or K <= 0"; return CE_E_BADARG;
    }
    int rc = pg_check(h, "ce_vjp_qp_many_params", rows, map_ptr, map_code, map_k, map_val, nullptr, ce_vjp_qp_many_variant(h),
                      ": this template has no search-free elimination with a quadratic objective inside the kernels (ce_vjp_qp_many_variant < 0); use the dA entry points, or the *_many_params entry of its kind",
                      false);
    if (rc) return rc;
    const long rpitch = (long)h->T.m + 1 + h->T.n;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(h->d_rec.reserve((size_t)K * B * rpitch));
    rc = vjp_qp_many_run(h, "ce_vjp_qp_many_params", B, K, A_vals_bm, sA_b, P_vals, x, y, s, dx, dy, nullptr, dq_vals, nullptr, adj_status, stream, h->d_rec.get(), rpitch);
    if (rc) return rc;
    return pg_records_launch(h, "ce_vjp_qp_many_params", B, K, x, y, rows, map_ptr, map_code, map_k, map_val, g, dq_vals, adj_status, stream);
}

// `steps` launches of k_backward_ns<..., FWD, REF> (with P_vals, ce_refine_qp: <..., FWD, REF, QP>), one complete safeguarded Newton step each; the per-instance record
// (refine_status, steps_taken, resid) carries an instance's state from launch to launch on the device.  No re-solve list: a flagged instance keeps its point.
static int refine_ns(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b, const double *P_vals, double *x, double *y, double *s,
                     const int *status, int steps, int *refine_status, int *steps_taken, double *resid, void *stream, bool psd = false, bool psd_tri = false) {
    const bool qp = P_vals != nullptr;
    const std::string who = qp ? "ce_refine_qp" : (psd_tri ? "ce_refine_psd_tri" : (psd ? "ce_refine_psd" : "ce_refine"));
    const CePlan &P = h->plan;
    const DevT &T = h->T;
    if (qp) { const int rc = qp_ns_check(h, "ce_refine_qp"); if (rc) return rc; }
    else if (psd_tri) {  // (the opt-in entry point of templates with PSD blocks and triples: ce_refine and ce_refine_psd keep refusing them)
        if (P.psd_tri_ns_variant < 0) { g_err = "ce_refine_psd_tri: this template has no search-free elimination with PSD blocks and triples (it lacks a PSD block or an exponential / power cone, has a quadratic objective, n > 108, its footprint exceeds LDS, or CE_BWD_NS=0)"; return CE_E_UNSUPPORTED; }
    } else if (psd) {      // (the opt-in entry point of PSD templates: ce_refine itself keeps refusing them)
        if (P.psd_ns_variant < 0) { g_err = "ce_refine_psd: this template has no search-free elimination with PSD blocks (no PSD block, triples or a quadratic objective beside them, n > 108, its footprint exceeds LDS, or CE_BWD_NS=0)"; return CE_E_UNSUPPORTED; }
    } else {
        if (P.qp_native) { g_err = "ce_refine: not available with a quadratic objective inside the kernels; use the epigraph form (cone form) of the problem"; return CE_E_UNSUPPORTED; }
        if (P.ns_variant < 0 && P.tri_ns_variant < 0) { g_err = "ce_refine: this template has no search-free elimination (PSD / exponential / power cones, or n > 108)"; return CE_E_UNSUPPORTED; }
    }
    const bool tri = !qp && !psd && !psd_tri && P.ns_variant < 0;      // exponential / power triples: k_backward_ns<..., FWD, REF, TRI>
    const int variant = qp ? P.qp_ns_variant : (psd_tri ? P.psd_tri_ns_variant : (psd ? P.psd_ns_variant : (tri ? P.tri_ns_variant : P.ns_variant)));
    const size_t lds = qp ? P.qp_ns_lds : (psd_tri ? P.psd_tri_ns_lds : (psd ? P.psd_ns_lds : (tri ? P.tri_ns_lds : P.ns_lds)));
    if (B > 1 && sA_b != T.nnz_aug) { g_err = who + ": A_vals_bm must be contiguous batch-major rows"; return CE_E_BADARG; }
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    ProfScope ps(h, 1, st);
    CeBwdArgs ba{};
    ba.T = T; ba.T.lda = T.n; ba.Abm = A_vals_bm;
    for (int k = 0; k < steps; k++) {
        const NsRefine W{h->d_bpos.get(), q_vals, sq_k, sq_b, x, y, s, status, refine_status, steps_taken, resid, k == 0 ? 1 : 0};
        const int lrc = qp ? ce_launch_ns(variant, B, lds, st, ba, NsRefineQp{W, NsQp{P_vals, nullptr, h->d_pmap.get(), h->nnz_p}})
                      : psd_tri ? ce_launch_ns(variant, B, lds, st, ba, NsRefinePsdTri{W})
                      : psd ? ce_launch_ns(variant, B, lds, st, ba, NsRefinePsd{W})
                      : tri ? ce_launch_ns(variant, B, lds, st, ba, NsRefineTri{W}) : ce_launch_ns(variant, B, lds, st, ba, W);
        if (lrc) { g_err = "internal: no refinement kernel for the planned variant"; return CE_E_BADARG; }
    }
    HIPCHK(hipGetLastError());
    return CE_OK;
}
int ce_refine(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b, double *x, double *y, double *s,
              const int *status, int steps, int *refine_status, int *steps_taken, double *resid, void *stream) {
    if (!h || B <= 0 || !A_vals_bm || !q_vals || !x || !y || !s || !refine_status || !steps_taken || !resid || steps < 0) { g_err = "ce_refine: null argument or negative step count"; return CE_E_BADARG; }
    return refine_ns(h, B, A_vals_bm, sA_b, q_vals, sq_k, sq_b, nullptr, x, y, s, status, steps, refine_status, steps_taken, resid, stream);
}
int ce_refine_psd(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b, double *x, double *y, double *s,
                  const int *status, int steps, int *refine_status, int *steps_taken, double *resid, void *stream) {
    if (!h || B <= 0 || !A_vals_bm || !q_vals || !x || !y || !s || !refine_status || !steps_taken || !resid || steps < 0) { g_err = "ce_refine_psd: null argument or negative step count"; return CE_E_BADARG; }
    return refine_ns(h, B, A_vals_bm, sA_b, q_vals, sq_k, sq_b, nullptr, x, y, s, status, steps, refine_status, steps_taken, resid, stream, true);
}
int ce_refine_psd_tri(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b, double *x, double *y, double *s,
                      const int *status, int steps, int *refine_status, int *steps_taken, double *resid, void *stream) {
    if (!h || B <= 0 || !A_vals_bm || !q_vals || !x || !y || !s || !refine_status || !steps_taken || !resid || steps < 0) { g_err = "ce_refine_psd_tri: null argument or negative step count"; return CE_E_BADARG; }
    return refine_ns(h, B, A_vals_bm, sA_b, q_vals, sq_k, sq_b, nullptr, x, y, s, status, steps, refine_status, steps_taken, resid, stream, false, true);
}
int ce_refine_qp(ce_handle h, int B, const double *A_vals_bm, long sA_b, const double *q_vals, long sq_k, long sq_b, const double *P_vals, double *x, double *y, double *s,
                 const int *status, int steps, int *refine_status, int *steps_taken, double *resid, void *stream) {
    if (!h || B <= 0 || !A_vals_bm || !q_vals || !P_vals || !x || !y || !s || !refine_status || !steps_taken || !resid || steps < 0) { g_err = "ce_refine_qp: null argument or negative step count"; return CE_E_BADARG; }
    return refine_ns(h, B, A_vals_bm, sA_b, q_vals, sq_k, sq_b, P_vals, x, y, s, status, steps, refine_status, steps_taken, resid, stream);
}
int ce_ca_triples(ce_handle h, int B, int lp, double *U, double *roots, const int *active, void *stream) {
    if (!h || B <= 0 || !U || !roots || !active) { g_err = "null argument"; return CE_E_BADARG; }
    const int ntri = h->T.nep + h->T.np;
    if (ntri == 0) return CE_OK;
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_ca_triples, dim3(((size_t)B * ntri + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, h->T, lp, B, U, roots, active);
    HIPCHK(hipGetLastError());
    return CE_OK;
}
int ce_ca_triple_jac(ce_handle h, int B, const double *v, long ld_v, double *J, void *stream) {
    if (!h || B <= 0 || !v || !J) { g_err = "null argument"; return CE_E_BADARG; }
    const int ntri = h->T.nep + h->T.np;
    if (ntri == 0) return CE_OK;
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_ca_triple_jac, dim3(((size_t)B * ntri + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, h->T, B, v, ld_v, J);
    HIPCHK(hipGetLastError());
    return CE_OK;
}
int ce_ca_update(ce_handle h, int B, int lp, double *W, const double *UT, const double *U, const int *active, int norm_after, double alpha, void *stream) {
    if (!h || B <= 0 || !W || !UT || !U || !active) { g_err = "null argument"; return CE_E_BADARG; }
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_ca_update, dim3(B), dim3(NT), 0, (hipStream_t)stream, h->T.n + h->T.m + 1, lp, W, UT, U, active, norm_after, alpha);
    HIPCHK(hipGetLastError());
    return CE_OK;
}
int ce_ca_finish(ce_handle h, int B, int lp, int max_iters, const double *W, const double *UT, const double *U, const double *D,
                 const double *E, const double *b_hat, const double *c_hat, const double *sigma, const double *scale,
                 const int *active, int *status, int *iters, double *x, double *y, double *s, void *stream) {
    if (!h || B <= 0 || !W || !UT || !U || !x || !y || !s) { g_err = "null argument"; return CE_E_BADARG; }
    HIPCHK(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_ca_finish, dim3(B), dim3(NT), NW * 8 * 8, (hipStream_t)stream, h->T, lp, max_iters, W, UT, U, D, E, b_hat, c_hat, sigma, scale, active, status, iters, x, y, s);
    HIPCHK(hipGetLastError());
    return CE_OK;
}

extern "C++" {
template <bool ACC>
static int parammap_launch(int device, int B, int rows, int cols, const int *indptr, const int *indices, const double *vals,
                           const double *P, long ld_p, double *out, long ld_out, void *stream) {
    if (B <= 0 || rows <= 0 || !indptr || !P || !out) { g_err = "null argument"; return CE_E_BADARG; }   // indices / vals may be null for an all-zero map
    HIPCHK(hipSetDevice(device));
    hipStream_t st = (hipStream_t)stream;
    const size_t lds = (size_t)cols * sizeof(double);
    if (cols > 0 && lds <= 64 * 1024 && B >= 256) {          // source row fits LDS (2+ workgroups per CU) and the batch fills the chip
        static std::atomic<bool> attr_done[2][64];                 // per device (the attribute is per device); re-setting it is harmless, so a benign race at most repeats the call
        const int dslot = device & 63;
        if (!attr_done[ACC][dslot].load(std::memory_order_acquire)) {
            HIPCHK(hipFuncSetAttribute((const void *)k_parammap_lds<ACC>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
            attr_done[ACC][dslot].store(true, std::memory_order_release);
        }
        hipLaunchKernelGGL(k_parammap_lds<ACC>, dim3(B), dim3(512), lds, st, rows, cols, indptr, indices, vals, P, ld_p, out, ld_out);
    } else if (B >= 1024) {
        dim3 grid((rows + 255) / 256, (B + 3) / 4);
        hipLaunchKernelGGL((k_parammap<4, ACC>), grid, dim3(256), 0, st, rows, B, indptr, indices, vals, P, ld_p, out, ld_out);
    } else {
        dim3 grid((rows + 255) / 256, B);
        hipLaunchKernelGGL((k_parammap<1, ACC>), grid, dim3(256), 0, st, rows, B, indptr, indices, vals, P, ld_p, out, ld_out);
    }
    HIPCHK(hipGetLastError());
    return CE_OK;
}
}  // extern "C++"
int ce_parammap_apply(int device, int B, int rows, const int *indptr, const int *indices, const double *vals,
                      const double *P, long ld_p, double *out, long ld_out, void *stream) {
    return parammap_launch<false>(device, B, rows, 0, indptr, indices, vals, P, ld_p, out, ld_out, stream);
}
int ce_parammap_apply2(int device, int B, int rows, int cols, int accumulate, const int *indptr, const int *indices, const double *vals,
                       const double *P, long ld_p, double *out, long ld_out, void *stream) {
    return accumulate ? parammap_launch<true>(device, B, rows, cols, indptr, indices, vals, P, ld_p, out, ld_out, stream)
                      : parammap_launch<false>(device, B, rows, cols, indptr, indices, vals, P, ld_p, out, ld_out, stream);
}

int ce_set_profiling(ce_handle h, int enable) {
    if (!h) return CE_E_BADARG;
    h->prof = enable == 1 ? 7 : (enable > 1 ? (enable >> 1) & 7 : 0);      // 1: every kind; 2 / 4 / 8 (or sums): forward / adjoint / layout launches only
    if (h->prof) { while (h->ev_pool.size() < 2048) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) break; h->ev_pool.push_back(e); } }      // (created HERE, not in front of the timed launches)
    return CE_OK;
}
int ce_reset_profile(ce_handle h) {
    if (!h) return CE_E_BADARG;
    for (auto &v : h->ev) { for (auto &p : v) { h->ev_pool.push_back(p.first); h->ev_pool.push_back(p.second); } v.clear(); }      // (kept for the next scopes)
    return CE_OK;
}
int ce_get_profile(ce_handle h, int which, double *mean_ms, int *launches) {
    if (!h || which < 0 || which > 2) return CE_E_BADARG;
    double tot = 0; int nl = 0;
    for (auto &p : h->ev[which]) { HIPCHK(hipEventSynchronize(p.second)); float ms = 0; HIPCHK(hipEventElapsedTime(&ms, p.first, p.second)); tot += ms; nl++; }
    if (mean_ms) *mean_ms = nl ? tot / nl : 0.0;
    if (launches) *launches = nl;
    return CE_OK;
}
int ce_get_launch_info(ce_handle h, int *fl, int *bl, int *fm, int *bm) {
    if (!h) return CE_E_BADARG;
    const CePlan &P = h->plan;
    if (fl) *fl = (int)P.fwd_lds; if (bl) *bl = (int)P.bwd_lds; if (fm) *fm = P.fwd_mode; if (bm) *bm = P.bwd_mode;
    return CE_OK;
}
int ce_get_plan(ce_handle h, int *out, int n_out) {
    if (!h) { g_err = "null argument"; return CE_E_BADARG; }
    const CePlan &P = h->plan;
    const int v[] = {P.fwd_mode, P.f2_variant, P.rt_variant, P.wl ? 1 : 0, P.aa_ok ? 1 : 0, h->T.gen_blocked_f, P.qp_native ? 1 : 0,
                     P.bwd_mode, P.brt_variant, P.two_tile ? 1 : 0, P.ns_variant, h->T.gen_blocked_b, h->sp_r, h->sp_RP, h->last_fast, h->last_sa_fwd, h->last_sa_lsqr, P.tri_ns_variant};
    const int cnt = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; out && i < cnt && i < n_out; i++) out[i] = v[i];
    return cnt;
}

}  // extern "C"
