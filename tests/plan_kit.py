"""Edge discovery over the engine's launch plan (include/cone_engine.h ce_get_plan; test infrastructure).

A FAMILY maps one integer (the swept size) to a template shape (n, cones, pattern); a PLAN FUNCTION maps a swept value to the plan dict of an engine created
for that shape (create only, no solve) or None when the engine refuses the shape.  find_edges() walks the values in order and records every place where the
plan changes: the last value before and the first value after.  dedupe() keeps one edge per (plan before, plan after) pair.  The edge logic is host-only
(tests/test_plan_kit.py checks it on synthetic plan functions); plan_of() is the GPU side."""
from __future__ import annotations

import numpy as np

# fields that tell kernels apart; sp_r (the number of dense rows, which changes with every row of a small dense template) and last_fast, last_sa_fwd,
# last_sa_lsqr (call history) are not plan edges by themselves -- sp_RP is
EDGE_FIELDS = ("fwd_mode", "f2_variant", "rt_variant", "wl", "aa_ok", "gen_blocked_f", "qp_native",
               "bwd_mode", "brt_variant", "two_tile", "ns_variant", "gen_blocked_b", "sp_RP")


# per-instance templates: sp_RP selects among the shared-A kernels, which serve only batch-invariant A (the shared-A family) -- not an edge of theirs
INSTANCE_FIELDS = tuple(f for f in EDGE_FIELDS if f != "sp_RP")


def fields_for(family):
    return EDGE_FIELDS if family == SHARED_FAMILY[0] else INSTANCE_FIELDS


def key(plan, fields=EDGE_FIELDS):
    return None if plan is None else tuple((f, plan[f]) for f in fields)


def find_edges(plan_fn, values, fields=EDGE_FIELDS):
    """[(v_before, plan_before, v_after, plan_after)] for every change of key(plan) between consecutive values (a None plan -- shape refused -- counts as a
    plan of its own, so the first refused size is an edge too)."""
    edges = []
    prev_v = prev_p = None
    first = True
    for v in values:
        p = plan_fn(v)
        if not first and key(p, fields) != key(prev_p, fields):
            edges.append((prev_v, prev_p, v, p))
        prev_v, prev_p, first = v, p, False
    return edges


def dedupe(edges, fields=EDGE_FIELDS):
    """one edge per (plan before, plan after) pair, the first one met"""
    seen, out = set(), []
    for e in edges:
        k = (key(e[1], fields), key(e[3], fields))
        if k not in seen:
            seen.add(k)
            out.append(e)
    return out


def edge_shapes(edges):
    """the values on both sides of the edges, each once, in order; refused shapes (plan None) dropped"""
    out = []
    for vb, pb, va, pa in edges:
        for v, p in ((vb, pb), (va, pa)):
            if p is not None and v not in out:
                out.append(v)
    return out


# ---------------------------------------------------------------------------------------------- families
def _zl(n, m, z):
    return n, {"z": z, "l": m - z, "q": []}


def _soc(n, m, q):
    """z = 0, the SOC blocks q, the remaining rows nonnegative"""
    q = [d for d in q]
    while sum(q) > m - 1:
        q.pop()
    return n, {"z": 0, "l": m - sum(q), "q": q}


# name -> (values, v -> (n, cones) or (n, cones, P-structure flag)); the sizes keep m >= n (bounded problems) and reach every residency mode
FAMILIES = {
    # zero + nonnegative rows: n swept at m = 24 and m = 200, m swept at n = 12
    "zl_n_m24": (range(1, 24), lambda n: _zl(n, 24, 4)),
    "zl_n_m200": (range(1, 200), lambda n: _zl(n, 200, 20)),
    "zl_m_n12": (range(12, 530), lambda m: _zl(12, m, 2)),
    # second-order cones no larger than SOC_SMALL = 32, and one larger
    "soc_small_n_m96": (range(1, 96), lambda n: _soc(n, 96, [4, 6, 8, 10, 12, 16, 20])),
    "soc_small_m_n16": (range(16, 300), lambda m: _soc(16, m, [5] * (m // 10))),
    "soc_big_n_m120": (range(1, 120), lambda n: (n, {"z": 0, "l": 120 - 40 - 8, "q": [40, 8]})),
    "soc_big_m_n20": (range(40, 300), lambda m: (20, {"z": 2, "l": m - 2 - 33, "q": [33]})),
    # mixed z / l / q: cones that fit every wave window of k_fwd2 (W = 64 / CHA >= 8), and a cone of 20 rows that does not fit a window of 8 or 16
    "mixed_wl_n_m64": (range(1, 64), lambda n: (n, {"z": 3, "l": 33, "q": [4, 7, 3, 6, 8]})),
    "mixed_wl_m_n10": (range(20, 200), lambda m: (10, {"z": 2, "l": m - 2 - 18, "q": [3, 7, 8]})),
    "mixed_nowl_n_m64": (range(1, 64), lambda n: (n, {"z": 3, "l": 33, "q": [20, 8]})),
    # PSD: n swept with one 4 x 4 block; the order swept at n = 12
    "psd_n": (range(1, 80), lambda n: (n, {"z": 1, "l": n + 4, "q": [], "s": [4]})),
    "psd_k": (range(2, 24), lambda k: (12, {"z": 1, "l": 12, "q": [], "s": [k]})),
    # exponential / power triples
    "exp_pow_n": (range(1, 90), lambda n: (n, {"z": 1, "l": n + 2, "q": [3], "ep": 3, "p": [0.3, -0.6]})),
    # native quadratic objective (template with a dense upper-triangular P structure)
    "qp_n": (range(1, 90), lambda n: (n, {"z": 0, "l": 2 * n, "q": []}, True)),
    "qp_n_l4": (range(50, 110), lambda n: (n, {"z": 0, "l": n + 4, "q": []}, True)),
}

# families swept for the coverage ledger only (create, no parity): shapes whose solution is not unique (m < n: k_backward_rt variant 4 is the worst-case
# tile only when n > 64 and n + m < 112) or too large for the oracle at test time (the size-generic forward with A and G in global memory whose
# column panel no longer fits LDS)
LEDGER_FAMILIES = {
    "wide_n_m40": (range(40, 120), lambda n: (n, {"z": 5, "l": 35, "q": []})),
    "zl_n_m700": (range(440, 700, 2), lambda n: (n, {"z": 20, "l": 680, "q": []})),
}

# shared-A templates: v dense rows (all n columns) + one bound row per variable (single entries): sp_RP 16 / 32 / 64 / 0
SHARED_FAMILY = ("shared_dense_rows", range(1, 72))
SHARED_N = 8
# the same rows followed by one more cone whose rows have a single entry each (the split's dense rows stay the first v): the cone sets that tell the
# instantiations of the shared-A kernels apart (csrc/ce_variants.h CE_SA_FWD_VARIANTS, CE_SA_LSQR_VARIANTS).  Not swept: sp_RP depends on v alone.
SHARED_CONE_SETS = {SHARED_FAMILY[0]: {}, SHARED_FAMILY[0] + "+psd3": {"s": [3]}, SHARED_FAMILY[0] + "+exp": {"ep": 1}}


def shape_of(family, v):
    """(n, cones, pattern or None, P structure (indices, indptr) or None)"""
    if family in SHARED_CONE_SETS:
        n = SHARED_N
        extra = SHARED_CONE_SETS[family]
        ne = sum(k * (k + 1) // 2 for k in extra.get("s", [])) + 3 * extra.get("ep", 0)
        cones = {"z": 0, "l": v + n, "q": [], **extra}
        pat = np.zeros((v + n + ne, n), dtype=bool)
        pat[:v] = True
        pat[v + np.arange(n), np.arange(n)] = True
        pat[v + n + np.arange(ne), np.arange(ne) % n] = True
        return n, cones, pat, None
    out = {**FAMILIES, **LEDGER_FAMILIES}[family][1](v)
    n, cones = out[0], out[1]
    pstruct = None
    if len(out) > 2 and out[2]:
        rows = np.concatenate([np.arange(j + 1) for j in range(n)]).astype(np.int32)
        ptr = np.concatenate([[0], np.cumsum(np.arange(1, n + 1))]).astype(np.int32)
        pstruct = (rows, ptr)
    return n, cones, None, pstruct


def family_values(family):
    return SHARED_FAMILY[1] if family == SHARED_FAMILY[0] else {**FAMILIES, **LEDGER_FAMILIES}[family][0]


def all_families(ledger=False):
    return list(FAMILIES) + [SHARED_FAMILY[0]] + (list(LEDGER_FAMILIES) if ledger else [])


def variant_rows(name):
    """the rows of a variant list of csrc/ce_variants.h (e.g. "CE_SA_LSQR_VARIANTS") as tuples of ints, the row index first"""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cvxpylayers_amd", "csrc", "ce_variants.h")).read()
    body = re.search(r"#define " + name + r"\(X\)((?:\s*\\\n\s*X\([^)]*\))+)", hdr).group(1)
    return [tuple(int(t) for t in row.split(",")) for row in re.findall(r"X\(([^)]*)\)", body)]


def plan_of(family, v, device=None):
    """Creates (and frees) an engine for the shape; its plan dict, or None when ce_create refuses the shape (CE_E_TOO_LARGE / UNSUPPORTED)."""
    import torch
    from cvxpylayers_amd import _lib, problems as P
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    n, cones, pat, pstruct = shape_of(family, v)
    tpl = P.dense_template(n, cones, pattern=pat)
    try:
        eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, device or torch.device("cuda", 0), p_structure=pstruct)
    except (NotImplementedError, _lib.EngineError):
        return None
    p = eng.plan()
    del eng
    return p
