"""Planted KKT points for the PSD-bearing modes of the search-free elimination at the edges of their two planners (csrc/ce_plan.h psd_ns_variant,
psd_tri_ns_variant) and at the smallest shapes at which each part of the blocks' LDS layout exists: tests/test_psd_edge_kit.py proves the inputs without a GPU,
tests/test_gpu_psd_mode_edges.py runs the eight modes on them.  Host only.

A KIND is "psd" (PSD blocks beside plain cones: ce_jvp_psd, ce_refine_psd, ce_vjp_psd_many, ce_jvp_psd_many) or "mixed" (blocks AND exponential / power triples: the
ce_*_psd_tri* entries).  A SHAPE is (kind, n, cones, states of the second-order blocks, positive eigenvalues per PSD block).

Points.  ns_edge_kit.plant's rule with the blocks counted in: A = N(0, 1) / sqrt(n), x and v drawn, y = Pi_K*(v), s = y - v, b = A x + s, c = -A^T y.  Block c of
order k with p = block_pos[c] positive eigenvalues has v_c = svec(Q diag(lambda) Q^T), Q a random orthogonal matrix (QR of a Gaussian one), |lambda| uniform in
[0.3, 1.3], the first p positive: p = k is a block inside the cone (D = I), p = 0 one inside the polar cone (D = 0), anything between has p (k - p) weighted rows with
B_ab = l+ / (l+ - l-) in [0.19, 0.81].  Such a block adds p (p + 1) / 2 unit directions and p (k - p) directions with an eigenvalue in (0, 1) to the rule that picks
the number of active nonnegative rows; zero, nonnegative and second-order rows and the triples' redraw loop are ns_edge_kit.plant's own.  y of a block is formed from
the planted (Q, lambda), the regularity check projects with psd_tri_ns_kit.proj (numpy.linalg.eigh): two routes.

Edges.  Families that step one size at a time (FAMILIES) are walked on the g++ build of the plan (psd_ns_kit.host_plan / psd_tri_ns_kit.host_plan) until the kind
is refused; both sides of every change of the kind's row are cases.  A refusal is attributed to its gate by calling resolve_lds_fits and ns_first_fit through the
shim below (GATES): "resolve" (the LSQR vectors of the re-solve), "columns" (4 ceil(n / 4) + 1 columns fit no row) or "footprint" (ns_layout with the blocks'
segments exceeds LDS on every row that holds the columns).

Reference uncertainty (reference_uncertainty(): the largest change of dense_jvp's answer, relative to 1 + max |answer|, when every entry of v moves by 1e-15
relative), measured on the CPU on every compared shape: at most 3.9e-13 (block_only:psd; order[26] 1.2e-14 psd / 1.1e-14 mixed, l[635]:psd 1.2e-14, l[631]:mixed
2.3e-14, triples[178]:mixed 8.9e-15) -- no shape's reference is less certain than 1e-9, so the median bound stays 1e-8 everywhere (median_bound();
tests/test_psd_edge_kit.py prints the figure per shape and asserts the bound)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import ns_edge_kit as E
import plan_kit as pk
import psd_many_kit as MK
import psd_ns_kit as PK
import psd_tri_ns_kit as TK
from cvxpylayers_amd import problems as P

KIND_FIELDS = {"psd": ("psd_ns_variant", "psd_ns_lds"), "mixed": ("psd_tri_ns_variant", "psd_tri_ns_lds")}
GATES = ("resolve", "columns", "footprint")
SWEEP_END = 1400          # no kind is served past this value of any family (asserted by family_values)
KC = 4
REF_OF = {0: 0, 1: 1, 3: 0}          # position of a right-hand side in a K = 4 call -> Gaussian draw (position 2 is the zero one): test_gpu_ns_many_edges.py's pattern
ZERO_AT, REPEAT_AT = 2, 3
MIN_REGULAR = 0.8
TRIPLE_MARGIN = 0.02          # a triple is redrawn until its interior eigenvalue is this far from 0 and 1: 2000 x NS_TRI_STIFF
_CACHE: dict = {}


def _tri(kind, **kw):
    return kw if kind == "mixed" else {}


def _spread(count):
    """positive eigenvalues of `count` blocks of order 3: every fourth one mixed (p = 1), the others outside, so that the unit directions stay below n = 24 and the
    weighted rows are spread over every wave's turn at the per-wave scratch"""
    return tuple(1 if c % 4 == 0 else 0 for c in range(count))


# name -> (kinds, first value, (kind, value) -> shape)
FAMILIES = {
    "n": (("psd", "mixed"), 12, lambda k, n: (k, n, {"z": 3, "l": n + 10, "q": [6], "s": [4, 3], **_tri(k, ep=1, p=[0.4])}, ("bd",), (2, 1))),
    "l": (("psd", "mixed"), 30, lambda k, l: (k, 24, {"z": 2, "l": l, "q": [], "s": [4], **_tri(k, ep=1, p=[])}, (), (2,))),
    "order": (("psd", "mixed"), 3, lambda k, o: (k, 24, {"z": 2, "l": 30, "q": [], "s": [o], **_tri(k, ep=1, p=[])}, (), (2,))),
    "count": (("psd", "mixed"), 1, lambda k, c: (k, 24, {"z": 2, "l": 30, "q": [], "s": [3] * c, **_tri(k, ep=1, p=[])}, (), _spread(c))),
    "triples": (("mixed",), 1, lambda k, t: (k, 24, {"z": 2, "l": 30, "q": [], "s": [4], "ep": t, "p": []}, (), (2,))),
}


def _waves(row):
    return pk.variant_rows("CE_NS_VARIANTS")[row][2] // 64


def _both(fn):
    return {k: fn(k) for k in KIND_FIELDS}


ROW_N = (12, 29, 61)          # an n on each row of CE_NS_VARIANTS for the shapes below (the CPU test asserts the rows)
# name -> {kind: shape}: the smallest shapes at which each thing exists
STRUCTURE = {
    "n1_s1": {"psd": ("psd", 1, {"s": [1]}, (), (1,))},                                                        # npad = 2; a block of order one is a nonnegative row
    "n2_s2": {"psd": ("psd", 2, {"s": [2]}, (), (1,)), "mixed": ("mixed", 2, {"s": [2], "ep": 1}, (), (1,))},
    "n3_l1_s21": {"psd": ("psd", 3, {"l": 1, "s": [2, 1]}, (), (1, 1))},
    "block_only": {"psd": ("psd", 5, {"s": [4]}, (), (2,))},
    "all_in": _both(lambda k: (k, 14, {"z": 1, "l": 6, "q": [4], "s": [3, 2], **_tri(k, ep=1)}, ("bd",), (3, 2))),          # D = I on every block
    "all_out_z_is_n": _both(lambda k: (k, 6, {"z": 6, "l": 3, "s": [3, 2], **_tri(k, ep=1)}, (), (0, 0))),             # D = 0, no active row, nothing to sweep
    "s_2_9": _both(lambda k: (k, 12, {"z": 1, "l": 8, "s": [2, 9], **_tri(k, ep=1)}, (), (1, 2))),                     # maxs = 9 pads the block of order 2
    **{f"blocks_over_waves_row{r}": _both(lambda k, r=r: (k, ROW_N[r], {"z": 3, "l": ROW_N[r] + 10, "s": [2] * (_waves(r) + 1), **_tri(k, ep=1)}, (), (1,) * (_waves(r) + 1)))
       for r in range(3)},
    "psd_rows_over_threads": _both(lambda k: (k, 24, {"z": 2, "l": 20, "s": [22, 3], **_tri(k, ep=1)}, (), (2, 1))),     # 259 PSD rows, 256 threads; the second block straddles
    "smallest_mixed": {"mixed": ("mixed", 2, {"s": [1], "ep": 1}, (), (0,))},
    "pow_and_block_no_plain_row": {"mixed": ("mixed", 4, {"s": [3], "p": [0.4]}, (), (1,))},
}
STRUCTURE_ROW = {**{f"blocks_over_waves_row{r}": r for r in range(3)}, "psd_rows_over_threads": 0}
# shapes without a nonnegative row to absorb the count: the triple is drawn on the boundary (one unit, one interior eigenvalue) -- or, where no unit direction is
# left, inside the polar cone
PLANT_ARGS = {"smallest_mixed": dict(triple_kinds={(1, 1)}), "pow_and_block_no_plain_row": dict(triple_kinds={(1, 1)})}


# ---------------------------------------------------------------------------------------------- planting
def batch_of(shape):
    return E.batch_of(shape[:3])


def plant(shape, B=None, seed=0, triple_kinds=None):
    """The planted batch of a shape: dict with A, b, c, x, y, s, v, cones, kind, n, m, Q and lam (per instance and block: the planted decomposition), and per
    instance k1 (unit directions), L (directions with an eigenvalue in (0, 1)), nf = n - k1"""
    kind, n, cones, q_states, block_pos = shape
    orders = list(cones.get("s", []))
    assert len(block_pos) == len(orders) and all(0 <= p <= k for p, k in zip(block_pos, orders)), shape
    assert (kind == "mixed") == (TK.ntri(cones) > 0) and orders, shape
    m = TK.m_of(cones)
    B = batch_of(shape) if B is None else B
    sub = {"z": cones.get("z", 0), "l": cones.get("l", 0), "q": list(cones.get("q", [])), "ep": cones.get("ep", 0), "p": list(cones.get("p", []))}
    base = E.plant(("tri" if kind == "mixed" else "plain", n, sub, q_states), B=B, seed=seed, triple_kinds=triple_kinds, triple_margin=TRIPLE_MARGIN,
                   extra_units=sum(p * (p + 1) // 2 for p in block_pos), extra_L=sum(p * (k - p) for p, k in zip(block_pos, orders)))
    o, d = TK.plain_rows(cones), TK.psd_rows(cones)
    rng = np.random.default_rng(seed + 104729)
    A = rng.standard_normal((B, m, n)) / np.sqrt(n)
    v = np.zeros((B, m)); y = np.zeros((B, m))
    v[:, :o], v[:, o + d:] = base["v"][:, :o], base["v"][:, o:]
    y[:, :o], y[:, o + d:] = base["y"][:, :o], base["y"][:, o:]
    Qs, lams = [], []
    for i in range(B):
        Qi, li = [], []
        for (r0, k), p in zip(TK.blocks(cones), block_pos):
            Q, _ = np.linalg.qr(rng.standard_normal((k, k)))
            lam = rng.uniform(0.3, 1.3, k) * np.where(np.arange(k) < p, 1.0, -1.0)
            v[i, r0:r0 + k * (k + 1) // 2] = PK.svec((Q * lam) @ Q.T)
            y[i, r0:r0 + k * (k + 1) // 2] = PK.svec((Q * np.maximum(lam, 0.0)) @ Q.T)
            Qi.append(Q); li.append(lam)
        Qs.append(Qi); lams.append(li)
    x = base["x"]
    s = y - v
    b = np.einsum("bij,bj->bi", A, x) + s
    c = -np.einsum("bij,bi->bj", A, y)
    return dict(shape=shape, kind=kind, n=n, m=m, cones=cones, A=A, b=b, c=c, x=x, y=y, s=s, v=v, Pm=None, Q=Qs, lam=lams, k1=base["k1"], L=base["L"], nf=n - base["k1"],
                triple_states=base["triple_states"], seed=seed)


def point(name, shape, **kw):
    """plant(shape) once per name: shared by the tests, not changed"""
    if ("pt", name) not in _CACHE:
        _CACHE[("pt", name)] = plant(shape, **kw)
    return _CACHE[("pt", name)]


def projections(pt):
    """[(y-hat, D)] of every instance by psd_tri_ns_kit.proj, cached in the point"""
    if "proj" not in pt:
        pt["proj"] = [TK.proj(pt["v"][i], pt["cones"]) for i in range(pt["x"].shape[0])]
    return pt["proj"]


def regularity(pt):
    """(condition of J, KKT residual relative to 1 + max(|b|, |c|)) of every instance with y-hat and D from psd_tri_ns_kit.proj (not the planted decomposition)"""
    if "cond" not in pt:
        B = pt["x"].shape[0]
        cond = np.zeros(B); res = np.zeros(B)
        for i, (yh, D) in enumerate(projections(pt)):
            J = TK.kkt_matrix(pt["A"][i], D)
            cond[i] = np.linalg.cond(J) if np.isfinite(J).all() else np.inf
            fx = pt["A"][i].T @ yh + pt["c"][i]; fy = pt["A"][i] @ pt["x"][i] + (yh - pt["v"][i]) - pt["b"][i]
            res[i] = max(np.abs(fx).max(), np.abs(fy).max()) / (1 + max(np.abs(pt["b"][i]).max(), np.abs(pt["c"][i]).max()))
        pt["cond"], pt["resid"] = cond, res
    return pt["cond"], pt["resid"]


def margins(pt):
    """(smallest min(B, 1 - B) of a weighted PSD row, smallest min(lambda, 1 - lambda) of a triple's interior eigenvalue) over the instances; 1.0 where there is none"""
    bm = tm = 1.0
    for i, (_, D) in enumerate(projections(pt)):
        bm = min(bm, PK.block_states(pt["v"][i], {**pt["cones"], "ep": 0, "p": []})[1])
        for ev in TK.triple_eigs(D, pt["cones"]):
            mix = ev[(ev >= E.EIG_SNAP) & (ev <= 1 - E.EIG_SNAP)]
            if mix.size:
                tm = min(tm, float(np.minimum(mix, 1 - mix).min()))
    return bm, tm


def stiff_constant():
    """NS_TRI_STIFF of csrc/ce_backward_ns.h"""
    import re
    src = open(os.path.join(pk.ROOT, "cvxpylayers_amd", "csrc", "ce_backward_ns.h")).read()
    return float(re.search(r"constexpr double NS_TRI_STIFF = ([0-9.eE+-]+);", src).group(1))


# ---------------------------------------------------------------------------------------------- right-hand sides and dense references
def tangents(pt, seed=1):
    return E.tangents(pt, seed)[:3]


def cotangents(pt):
    """(KC, B, n), (KC, B, m): two draws, the zero one, the first again"""
    rng = np.random.default_rng(pt["seed"] + 31)
    xb = np.zeros((KC,) + pt["x"].shape); yb = np.zeros((KC,) + pt["y"].shape)
    for k in (0, 1):
        xb[k] = rng.standard_normal(pt["x"].shape); yb[k] = rng.standard_normal(pt["y"].shape)
    xb[REPEAT_AT], yb[REPEAT_AT] = xb[0], yb[0]
    return xb, yb


def dense_jvp(pt, t, v=None):
    """(dx, dy, ds, well conditioned, condition numbers): psd_tri_ns_kit.dense_jvp at the planted point (v: at y = Pi(v), s = y - v of another v instead)"""
    y, s = pt["y"], pt["s"]
    if v is not None:
        y = np.array([TK.proj(v[i], pt["cones"])[0] for i in range(v.shape[0])]); s = y - v
    return TK.dense_jvp(pt["A"], pt["x"], y, s, *t, pt["cones"])


def want_forward(pt, d):
    """the dense forward derivative of Gaussian draw d (tangents(pt, d + 1)): once per point"""
    if ("fwd", d) not in pt:
        w = dense_jvp(pt, tangents(pt, d + 1))
        assert w[3].all(), (pt["shape"], w[4])          # nothing left out
        pt[("fwd", d)] = w[:3]
    return pt[("fwd", d)]


def want_adjoint(pt, d):
    """{"dA", "db", "dc"} of cotangent draw d by psd_many_kit.dense_adjoint with the mixed projection's D: once per point"""
    if ("adj", d) not in pt:
        xb, yb = cotangents(pt)
        g, cond = MK.dense_adjoint(pt["A"], pt["x"], pt["y"], pt["s"], xb[d], yb[d], pt["cones"], D=[D for _, D in projections(pt)])
        assert (cond <= 1e11).all() and np.isfinite(g["dA"]).all(), (pt["shape"], cond.max())          # nothing left out
        pt[("adj", d)] = g
    return pt[("adj", d)]


def reference_uncertainty(pt):
    """the largest change of dense_jvp's answer, relative to 1 + max |answer| per instance, when every entry of v moves by 1e-15 relative"""
    if "unc" not in pt:
        rng = np.random.default_rng(pt["seed"] + 5)
        v1 = pt["v"] * (1 + 1e-15 * rng.choice([-1.0, 1.0], pt["v"].shape))
        w0, w1 = want_forward(pt, 0), dense_jvp(pt, tangents(pt, 1), v=v1)
        pt["unc"] = float(max(rel(a, b).max() for a, b in zip(w1[:3], w0)))
    return pt["unc"]


def median_bound(pt):
    """1e-8, the project's bound -- or 100 x the reference's own uncertainty where that is above 1e-9"""
    u = reference_uncertainty(pt)
    return 1e-8 if u <= 1e-9 else 100 * u


def rel(got, want):
    """per instance: max |got - want| / (1 + max |want|)"""
    return np.abs(got - want).max(axis=-1) / (1 + np.abs(want).max(axis=-1))


def hold(tag, what, arrays, wants, reg, median_bd=1e-8, flagged_bound=True):
    """The comparison of one right-hand side, for every mode: arrays / wants the (B, .) outputs and their dense references, reg the status-0 instances.  Status 0:
    maximum 1e-5 and median median_bd relative to 1 + max |reference|; flagged (re-solved): median 1e-6, maximum 5e-3 (test_gpu_jvp_direct.py).  Returns (worst,
    median) over the status-0 instances, nan where there is none."""
    e = np.max([rel(g, w) for g, w in zip(arrays, wants)], axis=0)
    out = (float("nan"), float("nan"))
    if reg.any():
        out = (float(e[reg].max()), float(np.median(e[reg])))
        assert out[0] < 1e-5, f"{tag}: {what}: status-0 error {out[0]:.3e} (instance {int(np.nonzero(reg)[0][e[reg].argmax()])}) above 1e-5"
        assert out[1] < median_bd, f"{tag}: {what}: status-0 median error {out[1]:.3e} above {median_bd:.1e}"
    if (~reg).any() and flagged_bound:
        assert np.median(e[~reg]) < 1e-6 and e[~reg].max() < 5e-3, f"{tag}: {what}: flagged errors {e[~reg].tolist()} above median 1e-6 / maximum 5e-3"
    return out


def perturbed(pt, rel_=1e-6, seed=2):
    """(x', y', s', v'): every entry of the planted (x, v) moved by rel_ * N(0, 1) clipped to 3, relative to itself (ns_edge_kit.perturbed's rule: far inside the 0.3
    of the planted eigenvalues); y' = Pi_K*(v') by psd_tri_ns_kit.proj"""
    rng = np.random.default_rng(pt["seed"] + 7919 * seed)
    x1 = pt["x"] * (1 + rel_ * np.clip(rng.standard_normal(pt["x"].shape), -3, 3))
    v1 = pt["v"] * (1 + rel_ * np.clip(rng.standard_normal(pt["v"].shape), -3, 3))
    y1 = np.array([TK.proj(v1[i], pt["cones"])[0] for i in range(v1.shape[0])])
    return x1, y1, y1 - v1, v1


def dense_newton(pt, x1, v1):
    """(x, v) after one dense Newton step (psd_tri_ns_kit.dense_newton) from (x1, v1), and the well-conditioned flags"""
    dx, dv, ok = TK.dense_newton(pt["A"], pt["b"], pt["c"], x1, v1, pt["cones"])
    return x1 + dx, v1 + dv, ok


distance = E.distance


# ---------------------------------------------------------------------------------------------- the two planners and their gates on the host (g++, no GPU)
HOST_SRC = r'''
#include <cstdio>
#include "ce_plan.h"
extern "C" {
// out: resolve_lds_fits, ns_first_fit's row with the template's counts, its footprint, whether 4 ceil(n / 4) + 1 columns fit the last row, whether the footprint fits
// LDS on some row (the column rule aside), then the plan's psd_ns_variant, psd_ns_lds, psd_tri_ns_variant, psd_tri_ns_lds
int h_gates(const ce_template *tpl, long *out) {
    DevT T{}; std::vector<int> qoff, soff; CePlan P;
    plan_sizes(tpl, T, qoff, soff);
    const int rc = plan_engine(tpl, T, tpl->nnz_p, read_plan_env(), P);
    if (rc) return rc;
    int psdrows = 0;
    for (int c = 0; c < tpl->ns; c++) psdrows += tpl->s[c] * (tpl->s[c] + 1) / 2;
    const int ntri = T.nep + T.np;
    size_t lds = 0;
    out[0] = resolve_lds_fits(T, T.eoff - psdrows);
    out[1] = ns_first_fit(T, false, &lds, ntri, psdrows);
    out[2] = (long)lds;
    out[3] = 4 * ((T.n + 3) / 4) + 1 <= 16 * NS_ROWS[std::size(NS_ROWS) - 1].NTILE;
    out[4] = 0;
    for (const auto &R : NS_ROWS) {
        const size_t by = ntri > 0 ? bwd_ns_psd_tri_lds_bytes_of(T.n, T.m, T.nq, ntri, T.ns, T.maxs, psdrows, R.NTILE, R.NTHR) : bwd_ns_psd_lds_bytes_of(T.n, T.m, T.nq, T.ns, T.maxs, psdrows, R.NTILE, R.NTHR);
        if (by <= LDS_LIMIT) out[4] = 1;
    }
    out[5] = P.psd_ns_variant; out[6] = (long)P.psd_ns_lds; out[7] = P.psd_tri_ns_variant; out[8] = (long)P.psd_tri_ns_lds;
    return 0;
}
}
'''
GATE_FIELDS = ("resolve_fits", "first_fit", "first_fit_lds", "columns_fit", "footprint_fits", "psd_ns_variant", "psd_ns_lds", "psd_tri_ns_variant", "psd_tri_ns_lds")
HOST_MAIN = r'''
// one dense template per line of the grid: the gates and the plan, printed
static void one(int n, int z, int l, int nq, int *q, int ns, int *s, int ep, int np_, double *p) {
    int m = z + l + 3 * ep + 3 * np_;
    for (int k = 0; k < nq; k++) m += q[k];
    for (int k = 0; k < ns; k++) m += s[k] * (s[k] + 1) / 2;
    std::vector<int> indices, indptr(1, 0);
    for (int j = 0; j <= n; j++) { for (int i = 0; i < m; i++) indices.push_back(i); indptr.push_back((int)indices.size()); }
    ce_template t{};
    t.n = n; t.m = m; t.nnz_aug = (int)indices.size(); t.indices = indices.data(); t.indptr = indptr.data(); t.z = z; t.l = l; t.nq = nq; t.q = q; t.ns = ns; t.s = s;
    t.nep = ep; t.np = np_; t.p = p;
    long out[9]; const int rc = h_gates(&t, out);
    printf("%d", rc); for (int i = 0; rc == 0 && i < 9; i++) printf(" %ld", out[i]); printf("\n");
}
'''


def _compile(out, src_text, extra):
    src = os.path.join(os.path.dirname(out), os.path.basename(out) + ".cpp")
    with open(src, "w") as f:
        f.write(src_text)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-D__host__=", "-D__device__=", *extra, "-I", os.path.join(pk.ROOT, "cvxpylayers_amd", "csrc"),
                           "-I", os.path.join(pk.ROOT, "include"), "-o", out, src])
    return out


def host_lib():
    """the shim above, compiled once per process with g++ into a temporary directory (as psd_ns_kit.host_lib)"""
    if "lib" not in _CACHE:
        from cvxpylayers_amd import _lib
        _CACHE["dir"] = tempfile.TemporaryDirectory(prefix="psd_edge_host_")
        L = C.CDLL(_compile(os.path.join(_CACHE["dir"].name, "libpsd_edge_host.so"), HOST_SRC, ["-shared", "-fPIC"]))
        L.h_gates.argtypes = [C.POINTER(_lib.CeTemplate), C.POINTER(C.c_long)]
        _CACHE["lib"] = L
    return _CACHE["lib"]


def gates(shape):
    """{GATE_FIELDS} of a shape from the shim, or None when plan_engine refuses the template"""
    from cvxpylayers_amd import _lib
    n, cones = shape[1], shape[2]
    tpl = P.dense_template(n, cones)
    keep = [np.ascontiguousarray(tpl.indices, dtype=np.int32), np.ascontiguousarray(tpl.indptr, dtype=np.int32), np.ascontiguousarray(cones.get("q", []), dtype=np.int32),
            np.ascontiguousarray(cones.get("s", []), dtype=np.int32), np.ascontiguousarray(cones.get("p", []), dtype=np.float64)]
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))          # noqa: E731
    t = _lib.CeTemplate()
    t.n, t.m, t.nnz_aug, t.indices, t.indptr = int(tpl.n), int(tpl.m), int(keep[1][-1]), ip(keep[0]), ip(keep[1])
    t.z, t.l, t.nq, t.q, t.ns, t.s = int(cones.get("z", 0)), int(cones.get("l", 0)), len(keep[2]), ip(keep[2]), len(keep[3]), ip(keep[3])
    t.nep, t.np, t.p = int(cones.get("ep", 0)), len(keep[4]), keep[4].ctypes.data_as(C.POINTER(C.c_double))
    out = (C.c_long * len(GATE_FIELDS))()
    return dict(zip(GATE_FIELDS, out)) if host_lib().h_gates(C.byref(t), out) == 0 else None


def gate_of(shape):
    """the gate that refuses a shape its kind's row: one of GATES (in the plan's order: the re-solve is asked first), or None when the shape is served"""
    g = gates(shape)
    if g is None:
        return "create"
    if g[KIND_FIELDS[shape[0]][0]] >= 0:
        return None
    if not g["resolve_fits"]:
        return "resolve"
    assert g["first_fit"] == -1, (shape, g)
    return "columns" if not g["columns_fit"] else "footprint"


def host_plan(shape):
    """{"variant", "lds"} of the shape's kind from the kind's own kit (psd_ns_kit.host_plan / psd_tri_ns_kit.host_plan), None when the plan refuses the template"""
    key = ("plan", shape[0], shape[1], repr(sorted(shape[2].items())), tuple(os.environ.get(e) for e in PK.PLAN_ENV))
    if key not in _CACHE:
        p = (PK if shape[0] == "psd" else TK).host_plan(shape[1], shape[2])
        vf, lf = KIND_FIELDS[shape[0]]
        _CACHE[key] = None if p is None else {"variant": int(p[vf]), "lds": int(p[lf]) if p[vf] >= 0 else 0}
    return _CACHE[key]


def served(shape):
    p = host_plan(shape)
    return p is not None and p["variant"] >= 0


def family_values(fam, kind):
    """the swept values of a family: from its first value to the first one at which the kind is no longer served, that one included"""
    _, v, fn = FAMILIES[fam]
    seen = False
    while v < SWEEP_END:
        ok = served(fn(kind, v))
        yield v
        if seen and not ok:
            return
        seen, v = seen or ok, v + 1
    raise AssertionError(f"{fam}:{kind}: still served at {SWEEP_END}")


def edge_table():
    """[(family, kind, v_before, row_before, v_after, row_after, gate of the far side or None)] of every family and kind, from the host plan"""
    if "edges" not in _CACHE:
        out = []
        for fam, (kinds, _, fn) in FAMILIES.items():
            for kind in kinds:
                row = lambda v: host_plan(fn(kind, v))["variant"] if served(fn(kind, v)) else None          # noqa: E731
                for vb, rb, va, ra in pk.find_edges(lambda v: None if row(v) is None else {"row": row(v)}, family_values(fam, kind), ("row",)):
                    out.append((fam, kind, vb, -1 if rb is None else rb["row"], va, -1 if ra is None else ra["row"], gate_of(fn(kind, va)) if ra is None else None))
        _CACHE["edges"] = out
    return _CACHE["edges"]


def edge_cases():
    """{name: (shape, row or -1, gate)}: both sides of every edge, each shape once"""
    out = {}
    for fam, kind, vb, rb, va, ra, gate in edge_table():
        for v, r in ((vb, rb), (va, ra)):
            out.setdefault(f"{fam}:{kind}[{v}]", (FAMILIES[fam][2](kind, v), r, gate if r < 0 else None))
    return out


def structure_cases():
    return {f"{name}:{kind}": (shape, host_plan(shape)["variant"], None) for name, by in STRUCTURE.items() for kind, shape in by.items()}


def all_cases():
    if "cases" not in _CACHE:
        _CACHE["cases"] = {**edge_cases(), **structure_cases()}
    return _CACHE["cases"]


GROUPS = [f"{fam}:{kind}" for fam, (kinds, _, _) in FAMILIES.items() for kind in kinds] + [f"{name}:{kind}" for name, by in STRUCTURE.items() for kind in by]


def cases_of(group):
    """the cases of one "family:kind" (its edge shapes) or of one "structure shape:kind" """
    return {k: c for k, c in all_cases().items() if k == group or k.startswith(group + "[")}


def plant_args(name):
    return PLANT_ARGS.get(name.split(":")[0], {})


def case_point(name):
    return point(name, all_cases()[name][0], **plant_args(name))
