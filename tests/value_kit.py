"""Shared by test_value_host.py and test_gpu_value.py: the numpy statements of the optimal value and of its envelope-theorem derivatives, the shapes they are
checked on, and the bounds.  Nothing here needs a GPU.

At a solution (x, y) of   min c^T x + d + 1/2 x^T P x   s.t.  A x + s = b, s in K   (solver form):
    pobj = c^T x + d + 1/2 x^T P x,      dobj = -b^T y - 1/2 x^T P x + d,
    dp*/dA = y x^T,  dp*/db = -y,  dp*/dc = x,  dp*/dd = 1,  dp*/dP = 1/2 x x^T          (the partial derivatives of the Lagrangian: the envelope theorem).
In the boundary convention A_eval = [-A.data, b], q_eval = [c, d] (include/cone_engine.h): dp*/dA_eval[k] = -y_row x_col for an A entry, -y_row for a b entry.
A one-triangle P structure counts an off-diagonal entry twice (ce_vjp_qp's dP convention).

Everything is evaluated in np.longdouble, so that the reference's own rounding error (2^-64 per operation) is far below the bounds of the tests:
    scalars     |got - want| <= 4 L 2^-53 sum |terms|      for a sum of L terms (any summation order of L products has an error below (L + 1) 2^-53 sum |terms|);
    gradients   every entry within 4 ulp of the exact product (three factors: two roundings).
"""
from __future__ import annotations

import numpy as np

from cvxpylayers_amd import problems as P

LD = np.longdouble
U = 2.0 ** -53

# the three templates of the feature's CPU check (n, cones, seed): plain cones, a PSD block, exponential triples
HOST_TEMPLATES = {
    "plain": (12, {"z": 2, "l": 6, "q": [4, 5]}, 1),
    "psd": (4, {"z": 1, "l": 0, "q": [], "s": [3]}, 0),
    "exp": (6, {"z": 1, "l": 3, "q": [], "s": [], "ep": 2}, 3),
}

# kernel shapes (n, cones, B, seed, sparse): the smallest that reach every index path -- B = 1; nnz_aug = 221 (not a multiple of 64, several waves) at B = 5
# (one full workgroup of four instances and a ragged one) and B = 65 (crosses the 64-instance tile of the batch-minor layout); an empty column of A and
# structural zeros in b; a PSD block; exponential triples
KERNEL_SHAPES = {
    "tiny_b1": (3, {"z": 1, "l": 3, "q": []}, 1, 2, False),
    "dense_b5": (12, {"z": 2, "l": 6, "q": [4, 5]}, 5, 1, False),
    "dense_b65": (12, {"z": 2, "l": 6, "q": [4, 5]}, 65, 1, False),
    "sparse_b5": (12, {"z": 2, "l": 6, "q": [4, 5]}, 5, 1, True),
    "sparse_b65": (12, {"z": 2, "l": 6, "q": [4, 5]}, 65, 1, True),
    "psd": (4, {"z": 1, "l": 0, "q": [], "s": [3]}, 5, 0, False),
    "exp": (6, {"z": 1, "l": 3, "q": [], "s": [], "ep": 2}, 5, 3, False),
}
QP_SHAPE = (6, {"z": 2, "l": 4, "q": []}, 5, 4)


def sparse_patterns(n, cones, seed):
    """(pattern (m, n), b_pattern (m,)): about 60 % of A, column 3 of A EMPTY, and structural zeros in b on every third nonnegative row"""
    m = P.cone_rows(cones)
    rng = np.random.default_rng(seed + 500)
    pattern = rng.random((m, n)) < 0.6
    pattern[:, 3] = False
    pattern[np.arange(m), np.arange(m) % n] |= (np.arange(m) % n) != 3          # no empty row
    b_pattern = np.ones(m, bool)
    z, l = int(cones.get("z", 0)), int(cones.get("l", 0))
    b_pattern[z:z + l:3] = False
    return pattern, b_pattern


def sparse_instance(n, cones, B, seed):
    """P.generate on the sparse pattern, then b = 0 on the rows b_pattern leaves out (nonnegative-cone rows: they become the homogeneous rows A_i x <= 0).
    c = -A^T y0 keeps the dual feasible whatever b is, so an instance stays bounded; that it also stays feasible is asserted by the tests (the oracle solves
    every instance of the shapes above)."""
    pattern, b_pattern = sparse_patterns(n, cones, seed)
    A, b, c = P.generate(n, cones, B, seed=seed, pattern=pattern)
    b = b * b_pattern[None]
    return A, b, c, pattern, b_pattern


def entries(tpl):
    """(row, column) of every structural entry of [A_cvx | b_cvx] in the value order; column n: a b entry"""
    return np.asarray(tpl.indices), np.repeat(np.arange(tpl.n + 1), np.diff(tpl.indptr))


def one_triangle(p_rows, p_cols):
    p_rows, p_cols = np.asarray(p_rows), np.asarray(p_cols)
    return bool(len(p_rows)) and (bool((p_rows <= p_cols).all()) or bool((p_rows >= p_cols).all()))


def p_entries(struct):
    """(p_rows, p_cols, weight) of a CSC P structure (indices, indptr, shape): weight 1/2, or 1 for an off-diagonal entry of a one-triangle structure"""
    idx, ptr = np.asarray(struct[0]), np.asarray(struct[1])
    cols = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    w = np.where(one_triangle(idx, cols) & (idx != cols), 1.0, 0.5)
    return idx, cols, w


def _quad_terms(x, P_vals, struct):
    pr, pc, w = p_entries(struct)
    return LD(w)[None] * np.asarray(P_vals, LD) * x[:, pr] * x[:, pc]          # (B, nnz_p)


def objective(tpl, A_eval, q_eval, x, y, P_vals=None, struct=None):
    """pobj, dobj (B,) in longdouble, with the sum of |terms| and the number of terms of each (for the bound).  A_eval (nnz_aug, B), q_eval (n+1, B),
    x (B, n), y (B, m); P_vals (B, nnz_p) in the order of struct."""
    x, y = np.asarray(x, LD), np.asarray(y, LD)
    A_eval, q_eval = np.asarray(A_eval, LD), np.asarray(q_eval, LD)
    n = tpl.n
    lin = q_eval[:n].T * x                                                     # (B, n)
    d = q_eval[n]
    b_pos = np.arange(tpl.indptr[n], tpl.indptr[n + 1])
    bty = A_eval[b_pos].T * y[:, np.asarray(tpl.indices)[b_pos]]               # (B, #b entries)
    quad = _quad_terms(x, P_vals, struct) if P_vals is not None else np.zeros((x.shape[0], 0), LD)
    pobj = lin.sum(1) + d + quad.sum(1)
    dobj = -bty.sum(1) - quad.sum(1) + d
    p_abs = np.abs(lin).sum(1) + np.abs(d) + np.abs(quad).sum(1)
    d_abs = np.abs(bty).sum(1) + np.abs(d) + np.abs(quad).sum(1)
    return dict(pobj=pobj, dobj=dobj, pobj_abs=p_abs, dobj_abs=d_abs, pobj_terms=lin.shape[1] + 1 + quad.shape[1], dobj_terms=bty.shape[1] + 1 + quad.shape[1])


def value_jvp(tpl, x, y, tA_eval=None, tq_eval=None, tP_vals=None, struct=None):
    """(tangent (B,), sum |terms| (B,), number of terms): tc^T x + td + 1/2 x^T tP x - sum_k tA_eval[k] (y_row x_col | y_row)"""
    x, y = np.asarray(x, LD), np.asarray(y, LD)
    B, n = x.shape
    rows, cols = entries(tpl)
    parts = []
    if tA_eval is not None:
        xc = np.concatenate([x, np.ones((B, 1), LD)], axis=1)
        parts.append(-np.asarray(tA_eval, LD).T * y[:, rows] * xc[:, cols])
    if tq_eval is not None:
        parts.append(np.asarray(tq_eval, LD).T * np.concatenate([x, np.ones((B, 1), LD)], axis=1))
    if tP_vals is not None:
        parts.append(_quad_terms(x, tP_vals, struct))
    terms = np.concatenate(parts, axis=1) if parts else np.zeros((B, 0), LD)
    return terms.sum(1), np.abs(terms).sum(1), terms.shape[1]


def value_vjp(tpl, x, y, g, struct=None):
    """exact products in longdouble: dA_eval (nnz_aug, B), dq_eval (n+1, B), dP (B, nnz_p) or None"""
    x, y, g = np.asarray(x, LD), np.asarray(y, LD), np.asarray(g, LD)
    B = x.shape[0]
    rows, cols = entries(tpl)
    xc = np.concatenate([x, np.ones((B, 1), LD)], axis=1)
    dA = (-g[:, None] * y[:, rows] * xc[:, cols]).T
    dq = (g[:, None] * xc).T
    dP = None
    if struct is not None:
        pr, pc, w = p_entries(struct)
        dP = g[:, None] * LD(w)[None] * x[:, pr] * x[:, pc]
    return dA, dq, dP


def scalar_bound(n_terms, abs_sum):
    return 4.0 * n_terms * U * np.asarray(abs_sum, np.float64)


def assert_scalar(got, want, abs_sum, n_terms, what):
    err = np.abs(np.asarray(got, LD) - want).astype(np.float64)
    bound = scalar_bound(n_terms, abs_sum)
    print(f"{what}: max |got - want| = {err.max():.3e}, bound at that instance = {bound[np.argmax(err - bound)]:.3e} ({n_terms} terms)")
    assert (err <= bound).all(), (what, err, bound)


def assert_ulp(got, exact, what, ulps=4):
    """every entry of got (float64) within `ulps` ulp of the exact product (longdouble)"""
    got = np.asarray(got, np.float64)
    ref = np.asarray(exact, LD)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got.astype(LD) - ref).astype(np.float64)
    tol = ulps * np.spacing(np.abs(ref.astype(np.float64)))
    bad = err > tol
    print(f"{what}: max error in ulp = {float((err / np.spacing(np.abs(ref.astype(np.float64)))).max()) if got.size else 0.0:.2f} over {got.size} entries")
    assert not bad.any(), (what, int(bad.sum()), got[bad][:4], ref[bad][:4])


def canon_values(template, params):
    """(A_eval (nnz_aug, B), q_eval (n+1, B), P_eval (nnz_p, B) or None, p (B, Ptot+1)) of a CanonTemplate at numpy parameter values: each parameter either with
    its own shape or with one leading batch axis; flattened in Fortran order at its canonical columns, then the constant 1 (torch/cvxpylayer.py:84-141)"""
    shapes = [tuple(s) for s in template.param_shapes]
    Bs = [np.asarray(v).shape[0] for v, s in zip(params, shapes) if np.asarray(v).ndim == len(s) + 1]
    B = Bs[0] if Bs else 1
    p = np.zeros((B, template.n_params_total + 1)); p[:, -1] = 1.0
    for v, s, off in zip(params, shapes, template.col_offsets):
        v = np.asarray(v, float)
        if v.ndim == len(s):
            v = np.broadcast_to(v, (B,) + s)
        size = int(np.prod(s)) if len(s) else 1
        p[:, off:off + size] = np.stack([v[i].reshape(-1, order="F") for i in range(B)])
    A_eval = (template.A_map @ p.T)
    q_eval = (template.q_map @ p.T)
    P_eval = (template.P_map @ p.T) if template.P_map is not None else None
    return np.asarray(A_eval), np.asarray(q_eval), (np.asarray(P_eval) if P_eval is not None else None), p


def param_grads(template, dA_eval, dq_eval, dP_eval=None):
    """the envelope gradients pushed back through the template's maps: one (B,) + shape array per parameter (the transposed maps, Fortran un-flattening)"""
    g = np.asarray(dA_eval, np.float64).T @ template.A_map.toarray() + np.asarray(dq_eval, np.float64).T @ template.q_map.toarray()
    if dP_eval is not None:
        g = g + np.asarray(dP_eval, np.float64).T @ template.P_map.toarray()
    out = []
    for s, off in zip(template.param_shapes, template.col_offsets):
        s = tuple(s)
        size = int(np.prod(s)) if len(s) else 1
        out.append(np.stack([g[i, off:off + size].reshape(s, order="F") for i in range(g.shape[0])]))
    return out


def identity_template(n, cones, with_d=False, pattern=None, b_pattern=None):
    """a layer whose parameters ARE the solver-form data: A (m, n), b (m,), c (n,) [, d ()]; variables: the whole primal and the whole dual vector"""
    from cvxpylayers_amd.torch import VariableRecovery
    from cvxpylayers_amd.torch.templates import template_from_affine_builder
    m = P.cone_rows(cones)
    pat = np.ones((m, n)) if pattern is None else pattern.astype(float)
    bpat = np.ones(m) if b_pattern is None else b_pattern.astype(float)
    rec = [VariableRecovery(slice(0, n), None, (n,)), VariableRecovery(None, slice(0, m), (m,), source="dual")]
    if with_d:
        return template_from_affine_builder(lambda A, b, c, d: (A * pat, b * bpat, c, None, d), [(m, n), (m,), (n,), ()], cones, rec)
    return template_from_affine_builder(lambda A, b, c: (A * pat, b * bpat, c), [(m, n), (m,), (n,)], cones, rec)
