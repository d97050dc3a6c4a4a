// plan_host.cpp -- test infrastructure (tests/plan_kit.py host_build): ce_create's host half up to the plan (validated templates only) and the two shared-A selectors on
// the template's own split, around csrc/ce_plan.h, compiled with g++ -D__host__= -D__device__=.  A shared object for ctypes; with -DPLAN_WALK_MAIN the same file is a
// program that reads the commands of plan_kit.write_grid() and prints one line of numbers per call -- what plan_kit.run_grid() returns for the same commands.
// -DN_PLAN_FIELDS and -DENV_NAMES (the switches the walker clears) come from plan_kit.
#include <cstdio>
#include "ce_plan.h"
// what index_cones / index_csr_split (cone_engine.hip) take from ce_plan.h
struct Sizes {
    DevT T{}; int sp_r = 0, sp_RP = 0, psd_first = 0;
    explicit Sizes(const ce_template *tpl) {
        std::vector<int> qoff, soff;
        plan_sizes(tpl, T, qoff, soff);
        psd_first = soff[0];
        sp_RP = split_RP((int)dense_rows(tpl).size(), &sp_r);
    }
};
extern "C" {
int h_plan(const ce_template *tpl, long *out) {
    const Sizes S(tpl); CePlan P;
    const DevT &T = S.T; const int sp_r = S.sp_r, sp_RP = S.sp_RP, psd_first = S.psd_first;
    const int rc = plan_engine(tpl, T, tpl->nnz_p, read_plan_env(), P);
    if (rc) return rc;
    const long v[] = {P.fwd_mode, (long)P.fwd_lds, P.rt_variant, P.rt_lda, P.f2_variant, P.f2_ldg, P.wl, P.aa_ok, P.qp_native, P.f2_neumann, P.gen_blocked_f, P.gen_blocked_b,
                      P.bwd_mode, (long)P.bwd_lds, P.nkcap, P.ldk, P.brt_variant, P.two_tile, P.fast_forced, P.ns_variant, (long)P.ns_lds, P.qp_ns_variant, (long)P.qp_ns_lds,
                      sp_r, sp_RP, psd_first};
    for (size_t i = 0; i < sizeof v / sizeof v[0]; i++) out[i] = v[i];
    return 0;
}
void h_sa_fwd(const ce_template *tpl, int aa, long *out) {
    const Sizes S(tpl);
    const SaFwdSel s = sa_fwd_select(S.T, S.sp_r, S.sp_RP, aa != 0);
    out[0] = s.row; out[1] = (long)s.lds; out[2] = s.aa_w_lds;
}
void h_sa_lsqr(const ce_template *tpl, int lsqr_variant, int per_inst, int listed, int fwd, long *out) {
    const Sizes S(tpl);
    const SaLsqrSel s = sa_lsqr_select(S.T, S.sp_RP, S.psd_first, lsqr_variant, per_inst != 0, listed != 0, fwd != 0);
    out[0] = s.row; out[1] = (long)s.lds; out[2] = s.RP; out[3] = s.a_lds;
}
// the three planners of k_backward_ns (plan_kit.NS_FIELDS; outside the recorded table).  out: ns_variant, qp_ns_variant, tri_ns_variant, their three LDS sizes,
// resolve_lds_fits (the acceptance edge of ce_jvp that no plan field shows)
int h_plan_ns(const ce_template *tpl, long *out) {
    const Sizes S(tpl); CePlan P;
    const int rc = plan_engine(tpl, S.T, tpl->nnz_p, read_plan_env(), P);
    if (rc) return rc;
    const long v[] = {P.ns_variant, P.qp_ns_variant, P.tri_ns_variant, (long)P.ns_lds, (long)P.qp_ns_lds, (long)P.tri_ns_lds, resolve_lds_fits(S.T, S.psd_first) ? 1 : 0};
    for (size_t i = 0; i < sizeof v / sizeof v[0]; i++) out[i] = v[i];
    return 0;
}
// the members of the union region of the layout on row v (ce_ns_layout.h bwd_ns_union_doubles).  out: a, b, c in doubles, the region, NTILE, NTHR
int h_ns_union(int n, int m, int nq, int v, long *out) {
    if (v < 0 || v >= (int)std::size(NS_ROWS)) return -1;
    const int NTILE = NS_ROWS[v].NTILE, nqs = nq > 0 ? nq : 1, npad = n + (n & 1);
    out[0] = (long)nqs * npad + 2 * (64 * bwd_ns_nsl(NTILE) + 2); out[1] = 8 * bwd_ns_ldp(NTILE); out[2] = m + (m & 1) + npad;
    out[3] = bwd_ns_union_doubles(n, m, nqs, NTILE); out[4] = NTILE; out[5] = NS_ROWS[v].NTHR;
    return 0;
}
// pack_rows for a wave window of W rows: 1 and the packed order is checked to be a permutation of the rows, 0 when the template cannot be packed, -1 on a bad order
int h_pack_rows(const ce_template *tpl, int W) {
    std::vector<int> ko, krc, kq;
    if (!pack_rows(tpl, W, ko, krc, kq)) return 0;
    std::vector<int> seen(tpl->m, 0);
    for (int r : ko) { if (r < 0 || r >= tpl->m || seen[r]++) return -1; }
    return (int)ko.size() == tpl->m && (int)krc.size() == tpl->m && kq.back() == tpl->m ? 1 : -1;
}
}
#ifdef PLAN_WALK_MAIN
// commands, one per line:  T n z l ep pflag nq q.. ns s.. np p.. kind [pattern]  (kind 0: dense A; 1: the m x n pattern follows, row by row, as a string of 0 / 1; b dense;
// pflag: dense upper-triangular P)  |  E name=value ... (the switches in force; the others are cleared)  |  P  |  K W  |  F aa  |  L lsqr_variant per_inst listed fwd
int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    static const char *ENV[] = {ENV_NAMES};
    std::vector<int> indices, indptr, q, s, pidx, pptr; std::vector<double> pw;
    ce_template t{}; long out[32]; char cmd[8];
    while (fscanf(f, "%7s", cmd) == 1) {
        if (cmd[0] == 'T') {
            int n, z, l, ep, pflag, cnt, kind;
            if (fscanf(f, "%d %d %d %d %d", &n, &z, &l, &ep, &pflag) != 5) return 3;
            if (fscanf(f, "%d", &cnt) != 1) return 3; q.assign(cnt, 0); for (int &x : q) if (fscanf(f, "%d", &x) != 1) return 3;
            if (fscanf(f, "%d", &cnt) != 1) return 3; s.assign(cnt, 0); for (int &x : s) if (fscanf(f, "%d", &x) != 1) return 3;
            if (fscanf(f, "%d", &cnt) != 1) return 3; pw.assign(cnt, 0); for (double &x : pw) if (fscanf(f, "%lf", &x) != 1) return 3;
            int m = z + l + 3 * ep + 3 * (int)pw.size();
            for (int d : q) m += d;
            for (int k : s) m += k * (k + 1) / 2;
            std::vector<char> pat((size_t)m * n + 1, '1');
            if (fscanf(f, "%d", &kind) != 1 || (kind == 1 && (fscanf(f, "%s", pat.data()) != 1 || strlen(pat.data()) != (size_t)m * n))) return 3;
            indices.clear(); indptr.assign(1, 0);
            for (int j = 0; j <= n; j++) {
                for (int i = 0; i < m; i++) if (j == n || pat[(size_t)i * n + j] == '1') indices.push_back(i);
                indptr.push_back((int)indices.size());
            }
            pidx.clear(); pptr.assign(1, 0);
            for (int j = 0; pflag && j < n; j++) { for (int i = 0; i <= j; i++) pidx.push_back(i); pptr.push_back((int)pidx.size()); }
            t = ce_template{};
            t.n = n; t.m = m; t.nnz_aug = (int)indices.size(); t.indices = indices.data(); t.indptr = indptr.data(); t.z = z; t.l = l;
            t.nq = (int)q.size(); t.q = q.data(); t.ns = (int)s.size(); t.s = s.data(); t.nep = ep; t.np = (int)pw.size(); t.p = pw.data();
            if (pflag) { t.nnz_p = (int)pidx.size(); t.p_indices = pidx.data(); t.p_indptr = pptr.data(); }
        } else if (cmd[0] == 'E') {
            for (const char *e : ENV) unsetenv(e);
            char line[512];
            if (!fgets(line, sizeof line, f)) return 3;
            for (char *tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n")) { char *eq = strchr(tok, '='); if (!eq) return 3; *eq = 0; setenv(tok, eq + 1, 1); }
        } else if (cmd[0] == 'P') {
            const int rc = h_plan(&t, out);
            printf("%d", rc);
            for (int i = 0; rc == 0 && i < N_PLAN_FIELDS; i++) printf(" %ld", out[i]);
            printf("\n");
        } else if (cmd[0] == 'K') {
            int W; if (fscanf(f, "%d", &W) != 1) return 3;
            printf("%d\n", h_pack_rows(&t, W));
        } else if (cmd[0] == 'F') {
            int aa; if (fscanf(f, "%d", &aa) != 1) return 3;
            h_sa_fwd(&t, aa, out); printf("%ld %ld %ld\n", out[0], out[1], out[2]);
        } else if (cmd[0] == 'L') {
            int a, b, c, d; if (fscanf(f, "%d %d %d %d", &a, &b, &c, &d) != 4) return 3;
            h_sa_lsqr(&t, a, b, c, d, out); printf("%ld %ld %ld %ld\n", out[0], out[1], out[2], out[3]);
        } else return 3;
    }
    fclose(f);
    return 0;
}
#endif
