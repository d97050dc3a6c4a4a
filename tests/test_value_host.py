"""The optimal value and its envelope-theorem gradients, on the CPU alone: the formulas of value_kit.py against the oracle's adjoint and against central
differences of the oracle's value, and the Python of the feature that needs no device (return_value, objective_sign, the five-value template builder).

The adjoint route the feature replaces is  loss = c^T x  back-propagated through the solution map: oracle.adjoint_batch with the cotangent dx = c, dy = 0 gives the
indirect part; at a solution its dA, db ARE y x^T and -y (the envelope's), and its dc vanishes, so that the total dc is the direct part x."""
import dataclasses
import inspect

import numpy as np
import pytest

import ref_cases
import value_kit as vk
from cvxpylayers_amd import problems as P


def _oracle_point(n, cones, B, seed, eps=1e-10):
    from oracle import oracle
    A, b, c = P.generate(n, cones, B, seed=seed)
    ref = oracle.solve_batch(A, b, c, cones, eps=eps, max_iters=400000)
    assert (ref["status"] == 1).all(), ref["status"]
    return A, b, c, ref


@pytest.mark.parametrize("name", list(vk.HOST_TEMPLATES))
def test_envelope_formulas_equal_the_adjoint_route(name):
    from oracle import oracle
    n, cones, seed = vk.HOST_TEMPLATES[name]
    B = 4
    A, b, c, ref = _oracle_point(n, cones, B, seed)
    tpl = P.dense_template(n, cones)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    obj = vk.objective(tpl, A_eval, q_eval, ref["x"], ref["y"])
    gap = np.abs(obj["pobj"] - obj["dobj"]).astype(float)
    print("gap of c^T x to -b^T y:", gap.max())
    assert (gap <= 1e-8 * (1 + np.abs(obj["pobj"]).astype(float))).all(), gap
    adj = oracle.adjoint_batch(A, b, c, cones, ref["x"], ref["y"], ref["s"], c, np.zeros_like(ref["y"]), lsqr_atol=1e-14, lsqr_btol=1e-14, lsqr_iter_lim=40000)
    want_dA, want_dq, _ = vk.value_vjp(tpl, ref["x"], ref["y"], np.ones(B))
    got_dA, _ = tpl.values_from_dense(adj["dA"], adj["db"], adj["dc"])                    # boundary convention [-dA.data, db]
    rel = np.abs(got_dA - want_dA.astype(float)).max(axis=0) / np.abs(want_dA.astype(float)).max(axis=0)
    rel_c = np.abs(adj["dc"]).max(axis=1) / np.maximum(1.0, np.abs(ref["x"]).max(axis=1))
    print("adjoint route vs y x^T and -y:", rel.max(), " its dc (vanishes):", rel_c.max())
    assert rel.max() <= 1e-8 and rel_c.max() <= 1e-8, (rel, rel_c)
    assert np.array_equal(want_dq[:n].T.astype(float), ref["x"]) and (want_dq[n] == 1).all()          # the direct part: dc = x, dd = 1


@pytest.mark.parametrize("name", list(vk.HOST_TEMPLATES))
def test_envelope_formulas_equal_central_differences_of_the_oracles_value(name):
    from oracle import oracle
    n, cones, seed = vk.HOST_TEMPLATES[name]
    B = 3
    A, b, c, ref = _oracle_point(n, cones, B, seed, eps=1e-11)
    tpl = P.dense_template(n, cones)
    rng = np.random.default_rng(seed + 40)
    tA, tb, tc = rng.standard_normal(A.shape), rng.standard_normal(b.shape), rng.standard_normal(c.shape)
    tA_eval, tq_eval = tpl.values_from_dense(tA, tb, tc)
    an, scale, _ = vk.value_jvp(tpl, ref["x"], ref["y"], tA_eval, tq_eval)
    h = 1e-6

    def value(sign):
        r = oracle.solve_batch(A + sign * h * tA, b + sign * h * tb, c + sign * h * tc, cones, eps=1e-11, max_iters=400000)
        assert (r["status"] == 1).all()
        return np.einsum("bj,bj->b", c + sign * h * tc, r["x"])
    fd = (value(+1) - value(-1)) / (2 * h)
    err = np.abs(fd - an.astype(float))
    print("central differences vs envelope:", err.max(), "on a scale of", float(scale.max()))
    assert (err <= 1e-6 * scale.astype(float)).all(), (err, scale)


def test_kit_counts_an_off_diagonal_entry_of_a_one_triangle_structure_twice():
    n, B = 4, 3
    rng = np.random.default_rng(0)
    G = rng.standard_normal((B, n, n)); Pm = G @ G.transpose(0, 2, 1)
    x = rng.standard_normal((B, n)); y = np.zeros((B, 1)); g = rng.standard_normal(B)
    tpl = P.dense_template(n, {"z": 1, "l": 0, "q": []})
    A_eval = np.zeros((tpl.nnz_aug, B)); q_eval = np.zeros((n + 1, B))
    full = (np.tile(np.arange(n), n).astype(np.int32), (np.arange(n + 1) * n).astype(np.int32), (n, n))
    rows, ptr = [], [0]
    for j in range(n):
        rows.extend(range(j + 1)); ptr.append(len(rows))
    upper = (np.asarray(rows, np.int32), np.asarray(ptr, np.int32), (n, n))
    want = 0.5 * np.einsum("bi,bij,bj->b", x, Pm, x)
    for struct in (full, upper):
        pr, pc, _ = vk.p_entries(struct)
        vals = Pm[:, pr, pc]
        o = vk.objective(tpl, A_eval, q_eval, x, y, vals, struct)
        assert np.allclose(o["pobj"].astype(float), want, rtol=1e-13) and np.allclose(o["dobj"].astype(float), -want, rtol=1e-13)
        dP = vk.value_vjp(tpl, x, y, g, struct)[2].astype(float)
        dense = np.zeros((B, n, n))
        np.add.at(dense, (slice(None), pr, pc), dP)
        if struct is upper:          # one entry stands for both matrix entries: spread it back
            dense = 0.5 * (dense + dense.transpose(0, 2, 1))
        assert np.allclose(dense, 0.5 * g[:, None, None] * x[:, :, None] * x[:, None, :], rtol=1e-13)


def test_return_value_argument_handling():
    from cvxpylayers_amd.torch import CvxpyLayer
    import torch
    cs = ref_cases.case_ridge_unbatched()
    layer = CvxpyLayer(template=cs["template"])
    sig = inspect.signature(layer.forward)
    assert sig.parameters["return_value"].default is False and sig.parameters["return_value"].kind is inspect.Parameter.KEYWORD_ONLY
    F0, g0 = (torch.from_numpy(p) for p in cs["params"])
    for bad in ("yes", 1, None):
        with pytest.raises(TypeError, match="return_value"):
            layer(F0, g0, return_value=bad)
    # the argument is looked at before anything else, and a valid one reaches the same checks as before
    with pytest.raises(ValueError, match="A tensor must be provided for each CVXPY parameter"):
        layer(F0, return_value=True)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            layer(F0, g0, return_value=True)


def test_objective_sign():
    from cvxpylayers_amd.torch import CanonTemplate, CvxpyLayer
    tpl = ref_cases.case_ridge_unbatched()["template"]
    assert tpl.objective_sign == 1
    assert [f.name for f in dataclasses.fields(CanonTemplate)][-1] == "objective_sign"          # appended: positional construction of the older fields is unchanged
    assert CvxpyLayer(template=dataclasses.replace(tpl, objective_sign=-1)).template.objective_sign == -1
    for bad in (0, 2, -2):
        with pytest.raises(ValueError, match="objective_sign"):
            CvxpyLayer(template=dataclasses.replace(tpl, objective_sign=bad))


def test_optimal_value_is_exported_and_refuses_a_cpu_only_host():
    import torch
    from cvxpylayers_amd import interfaces
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx
    from cvxpylayers_amd.interfaces.optimal_value import optimal_value
    assert interfaces.optimal_value is optimal_value
    tpl = P.dense_template(3, {"z": 0, "l": 4, "q": []})
    ctx = MI355_ctx(None, tpl.problem_data_index, tpl.cones)
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            optimal_value(None, torch.zeros(4, 2, dtype=torch.double), torch.zeros(tpl.nnz_aug, 2, dtype=torch.double),
                          torch.zeros(2, 3, dtype=torch.double), torch.zeros(2, 4, dtype=torch.double), ctx)


def test_five_value_builder_puts_the_objective_constant_into_row_n_of_q_map():
    from cvxpylayers_amd.torch import VariableRecovery
    from cvxpylayers_amd.torch.templates import template_from_affine_builder
    n, cones = 3, {"z": 1, "l": 3, "q": []}
    m = P.cone_rows(cones)
    rng = np.random.default_rng(1)
    A0 = rng.standard_normal((m, n)); w = rng.standard_normal(n)
    rec = [VariableRecovery(slice(0, n), None, (n,))]
    shapes = [(m,), (n,)]
    three = template_from_affine_builder(lambda b, c: (A0, b, c), shapes, cones, rec)
    five = template_from_affine_builder(lambda b, c: (A0, b, c, None, 2.5 + w @ c - 3.0 * b[0]), shapes, cones, rec)
    # d = 2.5 + w^T c - 3 b_0: a constant column and parameter columns in row n; everything else as the three-value builder gives it
    assert five.q_map.shape == three.q_map.shape == (n + 1, m + n + 1)
    assert three.q_map.toarray()[n].tolist() == [0.0] * (m + n + 1)
    want = np.zeros(m + n + 1); want[0] = -3.0; want[m:m + n] = w; want[-1] = 2.5
    assert np.allclose(five.q_map.toarray()[n], want, rtol=1e-13, atol=1e-15)
    assert np.array_equal(five.q_map.toarray()[:n], three.q_map.toarray()[:n])
    assert np.array_equal(five.A_map.toarray(), three.A_map.toarray()) and five.P_map is None and five.P_structure is None
    for a, b_ in zip(five.A_structure[:2], three.A_structure[:2]):
        assert np.array_equal(a, b_)
    # a quadratic objective and a constant together; the four-value builder is untouched by the fifth slot
    Pm = np.diag([1.0, 2.0, 3.0])
    four = template_from_affine_builder(lambda b, c: (A0, b, c, Pm), shapes, cones, rec)
    both = template_from_affine_builder(lambda b, c: (A0, b, c, Pm, 1.0), shapes, cones, rec)
    assert np.array_equal(four.P_map.toarray(), both.P_map.toarray()) and np.array_equal(four.P_structure[0], both.P_structure[0])
    assert four.q_map.toarray()[n].tolist() == [0.0] * (m + n + 1) and both.q_map.toarray()[n, -1] == 1.0
    vals = vk.canon_values(five, [np.arange(m, dtype=float), np.ones(n)])
    assert np.isclose(vals[1][n, 0], 2.5 + w.sum())
