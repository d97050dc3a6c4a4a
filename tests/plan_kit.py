"""Edge discovery over the engine's launch plan (include/cone_engine.h ce_get_plan; test infrastructure).

A FAMILY maps one integer (the swept size) to a template shape (n, cones, pattern); a PLAN FUNCTION maps a swept value to the plan dict of an engine created
for that shape (create only, no solve) or None when the engine refuses the shape.  find_edges() walks the values in order and records every place where the
plan changes: the last value before and the first value after.  dedupe() keeps one edge per (plan before, plan after) pair.  The edge logic is host-only
(tests/test_plan_kit.py checks it on synthetic plan functions); plan_of() is the GPU side.

The plan itself makes no HIP call (csrc/ce_plan.h), so it also runs on the host: host_lib() compiles that header with g++ behind a small C shim, host_plan_of() is
plan_of() without a GPU, and plan_grid() / run_grid() walk the grid of tests/golden/plan_table.json (tests/test_plan_host.py, tests/golden/make_plan_table.py)."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import tempfile

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


# ---------------------------------------------------------------------------------------------- the plan on the host (csrc/ce_plan.h compiled with g++)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the whole CePlan, then what index_csr_split / index_cones derive beside it (sp_r, sp_RP: ce_get_plan reports them; psd_first: sa_lsqr_select reads it)
PLAN_FIELDS = ("fwd_mode", "fwd_lds", "rt_variant", "rt_lda", "f2_variant", "f2_ldg", "wl", "aa_ok", "qp_native", "f2_neumann", "gen_blocked_f", "gen_blocked_b",
               "bwd_mode", "bwd_lds", "nkcap", "ldk", "brt_variant", "two_tile", "fast_forced", "ns_variant", "ns_lds", "qp_ns_variant", "qp_ns_lds", "sp_r", "sp_RP", "psd_first")
SA_FWD_FIELDS = ("row", "lds", "aa_w_lds")
SA_LSQR_FIELDS = ("row", "lds", "RP", "a_lds")
# the create-time switches of tests/test_gpu_plan_edges.py (SWITCHES there is this list)
SWITCHES = [{}, {"CE_FWD": "rt"}, {"CE_FWD": "generic"}, {"CE_FORCE_GENERIC": "1"}, {"CE_BWD_NS": "0"}, {"CE_GEN_BLOCKED": "0"}, {"CE_WL": "0"},
            {"CE_FORCE_GENERIC": "1", "CE_GEN_BLOCKED": "0"}]
# the call-time switches of the shared-A selectors that test_gpu_plan_edges.py::sa_rows_at uses, and the two others sa_lsqr_select reads
SA_FWD_SWITCHES = [{}, {"CE_SA_NT": "512"}, {"CE_SA_NT": "512", "CE_SA_CIDX": "0"}, {"CE_SA_NT": "256"}]
SA_LSQR_SWITCHES = [{}, {"CE_SA_LSQR_SPEC": "0"}, {"CE_SA_SPLIT": "0"}, {"CE_LSQR_A_LDS": "0"}]
SA_DENSE_ROWS = (3, 20, 40)
PLAN_ENV = ("CE_FWD", "CE_FORCE_GENERIC", "CE_BWD_NS", "CE_GEN_BLOCKED", "CE_WL", "CE_F2_NEUMANN", "CE_BWD_TWO_TILE", "CE_BWD_FAST_VARIANT",
            "CE_SA_NT", "CE_SA_CIDX", "CE_SA_LSQR_SPEC", "CE_SA_SPLIT", "CE_LSQR_A_LDS", "CE_SA_LSQR_PADLDS")


def host_build(out_dir, program=False, extra=()):
    """compiles tests/plan_host.cpp (the shim around csrc/ce_plan.h) with g++ into out_dir: a shared object for ctypes, or (program) the stand-alone walker; its path"""
    out = os.path.join(str(out_dir), "plan_walk" if program else "libplan_host.so")
    mode = ["-DPLAN_WALK_MAIN", "-DENV_NAMES=" + ", ".join(f'"{e}"' for e in PLAN_ENV)] if program else ["-shared", "-fPIC"]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__host__=", "-D__device__=", f"-DN_PLAN_FIELDS={len(PLAN_FIELDS)}", *mode, *extra,
                           "-I", os.path.join(ROOT, "cvxpylayers_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", out, os.path.join(ROOT, "tests", "plan_host.cpp")])
    return out


_HOST = {}


def host_lib():
    """the g++ build of the plan, compiled once per process into a temporary directory"""
    if "lib" not in _HOST:
        _HOST["dir"] = tempfile.TemporaryDirectory(prefix="plan_host_")
        _HOST["lib"] = C.CDLL(host_build(_HOST["dir"].name))
    return _HOST["lib"]


def host_template(family, v):
    """(ce_template, the arrays it points to) of the shape"""
    from cvxpylayers_amd import _lib, problems as P
    n, cones, pat, pstruct = shape_of(family, v)
    tpl = P.dense_template(n, cones, pattern=pat)
    keep = [np.ascontiguousarray(tpl.indices, dtype=np.int32), np.ascontiguousarray(tpl.indptr, dtype=np.int32), np.ascontiguousarray(cones.get("q", []), dtype=np.int32),
            np.ascontiguousarray(cones.get("s", []), dtype=np.int32), np.ascontiguousarray(cones.get("p", []), dtype=np.float64)]
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    t = _lib.CeTemplate()
    t.n, t.m, t.nnz_aug, t.indices, t.indptr = int(tpl.n), int(tpl.m), int(keep[1][-1]), ip(keep[0]), ip(keep[1])
    t.z, t.l, t.nq, t.q, t.ns, t.s = int(cones.get("z", 0)), int(cones.get("l", 0)), len(keep[2]), ip(keep[2]), len(keep[3]), ip(keep[3])
    t.nep, t.np, t.p = int(cones.get("ep", 0)), len(keep[4]), keep[4].ctypes.data_as(C.POINTER(C.c_double))
    if pstruct is not None:
        keep += [np.ascontiguousarray(pstruct[0], dtype=np.int32), np.ascontiguousarray(pstruct[1], dtype=np.int32)]
        t.nnz_p, t.p_indices, t.p_indptr = int(keep[6][-1]), ip(keep[5]), ip(keep[6])
    return t, keep


def host_plan_of(family, v, lib=None):
    """plan_of() without a GPU: every PLAN_FIELDS entry (ce_get_plan's create-time fields among them) from the g++ build, or None when plan_engine refuses the
    shape.  The switches are read from the environment, as ce_create reads them."""
    t, keep = host_template(family, v)
    buf = (C.c_long * len(PLAN_FIELDS))()
    return dict(zip(PLAN_FIELDS, buf)) if (lib or host_lib()).h_plan(C.byref(t), buf) == 0 else None


# ---------------------------------------------------------------------------------------------- the three planners of k_backward_ns (tests/test_gpu_ns_mode_edges.py)
# Swept beside the families above and outside tests/golden/plan_table.json: the plain, QP and TRI footprints of csrc/ce_ns_layout.h differ (the dense P; the
# triples' W and lambda), so each kind has LDS edges of its own.  A KIND is "plain" | "qp" | "tri"; its field says which row of CE_NS_VARIANTS serves it.
NS_FIELDS = ("ns_variant", "qp_ns_variant", "tri_ns_variant")
NS_PLAN_FIELDS = NS_FIELDS + ("ns_lds", "qp_ns_lds", "tri_ns_lds", "resolve_fits")
NS_KIND_FIELD = {"plain": "ns_variant", "qp": "qp_ns_variant", "tri": "tri_ns_variant"}
NS_SWEEP_END = 1400          # no kind is served past this many rows or triples (asserted by ns_family_values)


def ns_shape(kind, n, rows, q=(), states=(), ep=0, p=()):
    """(kind, n, cones, states of the second-order blocks): `rows` zero + nonnegative + second-order rows (z = min(2, n // 4), the blocks q that fit, the rest
    nonnegative) and, TRI kind, ep exponential and len(p) power triples behind them"""
    z = min(2, n // 4)
    q, states = list(q), list(states)
    while q and z + sum(q) > rows - 1:
        q.pop(); states.pop()
    cones = {"z": z, "l": rows - z - sum(q), "q": q}
    if kind == "tri":
        cones.update(ep=ep, p=list(p))
    return kind, n, cones, tuple(states)


def _ns_n(kind):          # n swept at n + 8 plain rows: one second-order block on the boundary (the smallest n have none or a block of 3)
    tri = dict(ep=1, p=[0.4]) if kind == "tri" else {}
    return lambda n: ns_shape(kind, n, n + 8, *(([8], ["bd"]) if n >= 10 else ([3], ["bd"]) if n >= 2 else ([], [])), **tri)


def _ns_m(kind, n, states):          # plain rows swept at fixed n: two second-order blocks in the given states
    tri = dict(ep=2, p=[0.4]) if kind == "tri" else {}
    return lambda m: ns_shape(kind, n, m, [5, 4], states, **tri)


def _ns_n_wide_block(kind):          # n swept with ONE boundary block of n + 2 rows: n directions with an eigenvalue in (0, 1), so that about n / 2 columns stay free for the
    tri = dict(ep=1, p=[0.4]) if kind == "tri" else {}          # sweep (at n + 8 rows a regular point of a linear objective leaves it a handful: ns_edge_kit.py)
    return lambda n: ns_shape(kind, n, min(2, n // 4) + n + 2 + n // 2 + 4, [n + 2], ["bd"], **tri)


# name -> (kind, first value, value -> shape).  The values run from the first one until the kind is refused (ns_family_values)
NS_FAMILIES = {}
for _k in NS_KIND_FIELD:
    NS_FAMILIES[f"{_k}_n"] = (_k, 1, _ns_n(_k))
    if _k != "qp":          # (a quadratic objective leaves about n / 2 columns free in every family)
        NS_FAMILIES[f"{_k}_n_wide_block"] = (_k, 1, _ns_n_wide_block(_k))
    for _n, _st in ((12, ("bd", "in")), (40, ("bd", "out")), (80, ("bd", "bd"))):
        NS_FAMILIES[f"{_k}_m_n{_n}"] = (_k, _n + 12, _ns_m(_k, _n, _st))
NS_FAMILIES["qp_n_l2n"] = ("qp", 1, lambda n: ("qp", n, {"z": 0, "l": 2 * n, "q": []}, ()))
NS_FAMILIES["tri_count_n12"] = ("tri", 1, lambda k: ns_shape("tri", 12, 14, [4], ["bd"], ep=k))


def ns_pstruct(kind, n):
    """dense upper-triangular P structure of the QP kind (shape_of's)"""
    if kind != "qp":
        return None
    return (np.concatenate([np.arange(j + 1) for j in range(n)]).astype(np.int32), np.concatenate([[0], np.cumsum(np.arange(1, n + 1))]).astype(np.int32))


def host_ns_plan(shape, lib=None):
    """{NS_PLAN_FIELDS} of a shape from the g++ build (h_plan_ns of tests/plan_host.cpp), or None when plan_engine refuses the template"""
    from cvxpylayers_amd import _lib, problems as P
    kind, n, cones = shape[:3]
    ck = (kind, n, repr(sorted(cones.items())), tuple(os.environ.get(e) for e in PLAN_ENV))
    if lib is None and ck in _HOST.setdefault("ns_plans", {}):
        return _HOST["ns_plans"][ck]
    out = _host_ns_plan(kind, n, cones, lib, _lib, P)
    if lib is None:
        _HOST["ns_plans"][ck] = out
    return out


def _host_ns_plan(kind, n, cones, lib, _lib, P):
    tpl = P.dense_template(n, cones)
    keep = [np.ascontiguousarray(tpl.indices, dtype=np.int32), np.ascontiguousarray(tpl.indptr, dtype=np.int32), np.ascontiguousarray(cones.get("q", []), dtype=np.int32),
            np.ascontiguousarray(cones.get("p", []), dtype=np.float64)]
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))          # noqa: E731
    t = _lib.CeTemplate()
    t.n, t.m, t.nnz_aug, t.indices, t.indptr = int(tpl.n), int(tpl.m), int(keep[1][-1]), ip(keep[0]), ip(keep[1])
    t.z, t.l, t.nq, t.q = int(cones.get("z", 0)), int(cones.get("l", 0)), len(keep[2]), ip(keep[2])
    t.nep, t.np, t.p = int(cones.get("ep", 0)), len(keep[3]), keep[3].ctypes.data_as(C.POINTER(C.c_double))
    ps = ns_pstruct(kind, n)
    if ps is not None:
        t.nnz_p, t.p_indices, t.p_indptr = int(ps[1][-1]), ip(ps[0]), ip(ps[1])
    buf = (C.c_long * len(NS_PLAN_FIELDS))()
    return dict(zip(NS_PLAN_FIELDS, buf)) if (lib or host_lib()).h_plan_ns(C.byref(t), buf) == 0 else None


def ns_served(kind, plan):
    return plan is not None and plan[NS_KIND_FIELD[kind]] >= 0


def ns_family_values(family, plan_fn=host_ns_plan):
    """the swept values of a family: from its first value to the first one at which its kind is no longer served, that one included"""
    kind, v, fn = NS_FAMILIES[family]
    seen = False
    while v < NS_SWEEP_END:
        ok = ns_served(kind, plan_fn(fn(v)))
        yield v
        if seen and not ok:
            return
        seen, v = seen or ok, v + 1
    raise AssertionError(f"{family}: still served at {NS_SWEEP_END}")


def ns_edges(family, plan_fn=host_ns_plan):
    """find_edges of a family on its kind's field and resolve_fits: [(v_before, plan_before, v_after, plan_after)].  A plan in which the kind is not served counts
    as refused (None), whatever else it holds."""
    kind, _, fn = NS_FAMILIES[family]
    fields = (NS_KIND_FIELD[kind], "resolve_fits")

    def served_plan(v):
        p = plan_fn(fn(v))
        return p if ns_served(kind, p) else None
    return find_edges(served_plan, ns_family_values(family, plan_fn), fields)


def ns_union_members(n, m, nq, row, lib=None):
    """(a, b, c) of the union region on a row of CE_NS_VARIANTS, in doubles: {a_z, publication buffers} | the sweep buffers | {q, g}"""
    out = (C.c_long * 6)()
    assert (lib or host_lib()).h_ns_union(int(n), int(m), int(nq), int(row), out) == 0
    assert out[3] == max(out[:3])
    return tuple(out[:3])


def switch_key(sw):
    return ",".join(f"{k}={v}" for k, v in sorted(sw.items()))


def plan_grid():
    """The grid of tests/golden/plan_table.json as commands (see tests/plan_host.cpp): every value of every family under every entry of SWITCHES -> the plan and pack_rows at the
    three wave windows; the three shared cone sets at SA_DENSE_ROWS -> both selectors over the call kinds and their switches."""
    cmds = []
    for fam in all_families(ledger=True):
        for v in family_values(fam):
            cmds.append(("T", fam, v))
            for sw in SWITCHES:
                cmds += [("E", sw), ("P",)] + ([("K", W) for W in (8, 16, 32)] if not sw else [])
    for fam in SHARED_CONE_SETS:
        for v in SA_DENSE_ROWS:
            for sw in SA_FWD_SWITCHES:
                cmds += [("E", sw), ("T", fam, v)] + [("F", aa) for aa in (0, 1)]
            for sw in SA_LSQR_SWITCHES:
                cmds += [("E", sw), ("T", fam, v)]
                # (a re-solve list belongs to calls with per-instance values)
                cmds += [("L", var, per, listed, fwd) for var in (0, 1) for per in (0, 1) for listed in (0, 1) for fwd in (0, 1) if per or not listed]
    return cmds


def run_grid(cmds, lib=None):
    """[(command with its template and switches, result tuple)] of every calling command, through the shared object"""
    L = lib or host_lib()
    buf = (C.c_long * 32)()
    saved = {e: os.environ.pop(e, None) for e in PLAN_ENV}
    out, cur, t, sw = [], None, None, {}
    try:
        for c in cmds:
            if c[0] == "E":
                for e in PLAN_ENV:
                    os.environ.pop(e, None)
                os.environ.update(c[1]); sw = c[1]
            elif c[0] == "T":
                if cur != c[1:]:
                    cur, t = c[1:], host_template(*c[1:])
            else:
                if c[0] == "P":
                    rc = L.h_plan(C.byref(t[0]), buf); res = (rc,) + (tuple(buf[:len(PLAN_FIELDS)]) if rc == 0 else ())
                elif c[0] == "K":
                    res = (L.h_pack_rows(C.byref(t[0]), c[1]),)
                elif c[0] == "F":
                    L.h_sa_fwd(C.byref(t[0]), c[1], buf); res = tuple(buf[:3])
                else:
                    L.h_sa_lsqr(C.byref(t[0]), *c[1:], buf); res = tuple(buf[:4])
                out.append((cur + (switch_key(sw),) + c, res))
    finally:
        for e in PLAN_ENV:
            os.environ.pop(e, None)
        os.environ.update({e: v for e, v in saved.items() if v is not None})
    return out


def write_grid(cmds, path):
    """the commands as the stand-alone walker reads them"""
    with open(path, "w") as f:
        for c in cmds:
            if c[0] == "E":
                f.write("E " + " ".join(f"{k}={v}" for k, v in c[1].items()) + "\n")
            elif c[0] == "T":
                n, cones, pat, pstruct = shape_of(*c[1:])
                lists = [cones.get("q", []), cones.get("s", []), cones.get("p", [])]
                f.write(f"T {n} {cones.get('z', 0)} {cones.get('l', 0)} {cones.get('ep', 0)} {int(pstruct is not None)} "
                        + " ".join(" ".join(str(x) for x in [len(li)] + list(li)) for li in lists)
                        + (" 0\n" if pat is None else " 1 " + "".join("1" if x else "0" for x in pat.ravel()) + "\n"))
            else:
                f.write(" ".join(str(x) for x in c) + "\n")


# ---- tests/golden/plan_table.json.  Plans are kept as RUNS, the forward and the backward half of the plan apart (most switches touch one half): per family, half
# and switch set, the ranges of the swept value over which every field of the half but its sizes is constant, with those fields once and the size fields (LDS bytes among
# them) at the run's first and last value.  A switch set whose runs equal the default's is "=".  The other calls are few: their results column by column in the
# grid's order, runs of equal values folded to [value, count].
HALVES = {"fwd": (("rc", "fwd_mode", "rt_variant", "f2_variant", "f2_ldg", "wl", "aa_ok", "f2_neumann", "gen_blocked_f", "sp_RP"), ("fwd_lds", "rt_lda", "sp_r", "psd_first")),
          "bwd": (("rc", "qp_native", "gen_blocked_b", "bwd_mode", "brt_variant", "two_tile", "fast_forced", "ns_variant", "qp_ns_variant"), ("bwd_lds", "nkcap", "ldk", "ns_lds", "qp_ns_lds"))}
assert sorted(f for kinds, sizes in HALVES.values() for f in kinds[1:] + sizes) == sorted(PLAN_FIELDS)


def _split(res, half):
    """(the fields of the half that tell plans apart, its size fields) of a plan_engine result (a refused shape: its return code, zeros)"""
    d = dict(zip(("rc",) + PLAN_FIELDS, res))
    return [[int(d.get(f, 0)) for f in fields] for fields in HALVES[half]]


def _fold(col):
    out = []
    for x in col:
        if out and isinstance(out[-1], list) and out[-1][0] == x:
            out[-1][1] += 1
        elif out and out[-1] == x:
            out[-1] = [x, 2]
        else:
            out.append(x)
    return out


def _unfold(col):
    return [y for x in col for y in ([x[0]] * x[1] if isinstance(x, list) else [x])]


def encode_table(results):
    """results of run_grid -> the JSON object of the fixture"""
    plans, cols = {}, {}
    for (fam, v, sw, kind, *_), res in results:
        for half in HALVES if kind == "P" else ():
            runs = plans.setdefault(fam, {}).setdefault(half, {}).setdefault(sw, [])
            kinds, sizes = _split(res, half)
            if runs and runs[-1][2] == kinds:
                runs[-1][1], runs[-1][4] = v, sizes
            else:
                runs.append([v, v, kinds, sizes, sizes])
        for i, x in enumerate(res if kind != "P" else ()):
            cols.setdefault(kind, [[] for _ in res])[i].append(int(x))
    for by in (by for halves in plans.values() for by in halves.values()):
        by.update({sw: "=" for sw, runs in by.items() if sw and runs == by[""]})
    return {"fields": {**{h: {"kind": list(k), "size": list(z)} for h, (k, z) in HALVES.items()}, "K": ["packed"], "F": list(SA_FWD_FIELDS), "L": list(SA_LSQR_FIELDS)},
            "runs": "[first value, last value, kind fields, size fields at the first value, at the last]", "plans": plans,
            "columns": {k: [_fold(c) for c in v] for k, v in cols.items()}}


def table_differences(results, obj):
    """[(call, got, recorded)] where results of run_grid disagree with the fixture: the kind fields of every plan of the grid against its run, the size fields at both
    ends of every run, every other call result by result.  Also a run or a column the grid did not reach."""
    assert obj["fields"] == encode_table([])["fields"]
    cols = {k: list(zip(*[_unfold(c) for c in v])) for k, v in obj["columns"].items()}
    at, ends, diffs = {k: 0 for k in cols}, set(), []
    for key, res in results:
        fam, v, sw, kind = key[:4]
        for half in HALVES if kind == "P" else ():
            runs = obj["plans"][fam][half][sw]
            runs = obj["plans"][fam][half][""] if runs == "=" else runs
            i = next((i for i, r in enumerate(runs) if r[0] <= v <= r[1]), None)
            kinds, sizes = _split(res, half)
            if i is None or runs[i][2] != kinds:
                diffs.append((key, half, kinds, None if i is None else runs[i][2]))
            for end, want in ((0, 3), (1, 4)):
                if i is not None and v == runs[i][end]:
                    ends.add((fam, half, sw, i, end))
                    if runs[i][want] != sizes:
                        diffs.append((key, half, sizes, runs[i][want]))
        if kind != "P":
            want = cols[kind][at[kind]] if at[kind] < len(cols[kind]) else None
            at[kind] += 1
            if want != tuple(res):
                diffs.append((key, tuple(res), want))
    diffs += [((fam, half, sw, "run", i, end), None, "not reached") for fam, halves in obj["plans"].items() for half, by in halves.items() for sw, runs in by.items() if runs != "="
              for i in range(len(runs)) for end in (0, 1) if (fam, half, sw, i, end) not in ends]
    diffs += [((k, "calls"), at[k], len(cols[k])) for k in cols if at[k] != len(cols[k])]
    return diffs
