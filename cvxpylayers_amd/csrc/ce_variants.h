// ce_variants.h -- the instantiated variants of every kernel family with more than one, stated ONCE.  The launcher translation units
// expand a list into their `switch` and their set-attribute loop; the launch plan (ce_plan.h) expands the same list into its planning
// table.  A row's first entry is the variant index the planner, ce_get_plan and the tests' ledger name it by; for the tiled families the
// planner takes the FIRST row that fits, so the order of the rows is part of the plan (the shared-A families are selected by value).  The trailing 0 / 1 columns say for which kinds the
// row is instantiated: a 0 discards the launch at compile time and the planner skips the row for templates of that kind.
// Adding a variant: one row here, one ledger entry in tests/test_gpu_plan_edges.py::EXPECTED.
#pragma once

// k_fwd2 (ce_forward_v2.h):  X(index, CHT, T1, CHA, T2, CHG, TG, threads per workgroup, WL, QP)
//   WL: plain cones with rows packed wave-local;  QP: quadratic objective inside the kernel.  (Plain and PSD kinds: every row.)
#define CE_F2_VARIANTS(X) \
    X(0, 16, 2, 8, 2, 16, 2, 256, 1, 0) \
    X(1, 8, 8, 4, 8, 8, 4, 256, 1, 0) \
    X(2, 4, 26, 2, 26, 4, 14, 256, 1, 1) \
    X(3, 8, 20, 2, 32, 8, 8, 512, 1, 1) \
    X(4, 4, 30, 4, 26, 4, 26, 512, 1, 1)

// k_forward_rt (ce_forward_rt.h), NT2 threads per workgroup:  X(index, CH1, T1, TG, CH2, T2, VP, workgroups per CU)
#define CE_RT_VARIANTS(X) \
    X(0, 8, 13, 7, 4, 13, 160, 4) \
    X(1, 8, 16, 8, 4, 16, 208, 4) \
    X(2, 4, 32, 32, 4, 32, 272, 2)

// k_backward_rt (ce_backward_rt.h):  X(index, TI, TJ, TH, row residues BGR, PSD)
//   K tile BGR*TI x 16*TJ and H tile 16*TH per workgroup of BGR*16 threads;  PSD: also built with PSD / exponential / power cones.
//   (Rows 1, 2, 5 were added as first tiles of the two-tile plan, which serves plain cones only.)
#define CE_BRT_VARIANTS(X) \
    X(0, 4, 4, 4, 16, 1) \
    X(1, 5, 5, 4, 16, 0) \
    X(2, 6, 6, 4, 16, 0) \
    X(3, 7, 7, 4, 16, 1) \
    X(4, 7, 7, 7, 16, 1) \
    X(5, 5, 9, 7, 32, 0) \
    X(6, 7, 13, 7, 32, 1)

// k_backward_ns (ce_backward_ns.h), plain cones (the forward modes of its TRI kind: exponential / power triples beside them, on the same rows):  X(index, tiles of 16 reduced columns, threads per workgroup)
#define CE_NS_VARIANTS(X) \
    X(0, 2, 256) \
    X(1, 4, 256) \
    X(2, 7, 512)

// k_sa_fwd (ce_shared_a_fwd.h), shared-A forward:  X(index, RP, threads per workgroup, CIDX, HTRI)
//   RP: dense rows padded;  CIDX: the template's index arrays in LDS (512 threads only);  HTRI: exponential / power triples compiled in
//   (rows without CIDX serve every cone kind).  The host selects a row by these values (ce_plan.h sa_fwd_select): the order is free.
#define CE_SA_FWD_VARIANTS(X) \
    X(0, 16, 256, 0, 1) \
    X(1, 32, 256, 0, 1) \
    X(2, 64, 256, 0, 1) \
    X(3, 16, 512, 0, 1) \
    X(4, 32, 512, 0, 1) \
    X(5, 64, 512, 0, 1) \
    X(6, 16, 512, 1, 0) \
    X(7, 32, 512, 1, 0) \
    X(8, 64, 512, 1, 0) \
    X(9, 16, 512, 1, 1) \
    X(10, 32, 512, 1, 1) \
    X(11, 64, 512, 1, 1)

// k_sa_lsqr (ce_shared_a.h), LSQR adjoint and forward derivative:  X(index, RP, HPSD, HTRI, LSMR, FWD)
//   RP 0: products through the CSR / CSC structure (per-instance values, or no split);  HPSD / HTRI: PSD blocks / triples compiled in;
//   LSMR: Fong & Saunders' recurrences;  FWD: the forward derivative.  Selected by these values (ce_plan.h sa_lsqr_select).
//   (PSD without triples has no RP = 0 row: those calls run the general kernel.)
#define CE_SA_LSQR_VARIANTS(X) \
    X(0, 0, 1, 1, 0, 0) \
    X(1, 16, 1, 1, 0, 0) \
    X(2, 32, 1, 1, 0, 0) \
    X(3, 64, 1, 1, 0, 0) \
    X(4, 0, 0, 0, 0, 0) \
    X(5, 16, 0, 0, 0, 0) \
    X(6, 32, 0, 0, 0, 0) \
    X(7, 64, 0, 0, 0, 0) \
    X(8, 16, 1, 0, 0, 0) \
    X(9, 32, 1, 0, 0, 0) \
    X(10, 64, 1, 0, 0, 0) \
    X(11, 0, 1, 1, 1, 0) \
    X(12, 16, 1, 1, 1, 0) \
    X(13, 32, 1, 1, 1, 0) \
    X(14, 64, 1, 1, 1, 0) \
    X(15, 0, 0, 0, 0, 1) \
    X(16, 16, 0, 0, 0, 1) \
    X(17, 32, 0, 0, 0, 1) \
    X(18, 64, 0, 0, 0, 1) \
    X(19, 0, 1, 1, 0, 1) \
    X(20, 16, 1, 1, 0, 1) \
    X(21, 32, 1, 1, 0, 1) \
    X(22, 64, 1, 1, 0, 1)
