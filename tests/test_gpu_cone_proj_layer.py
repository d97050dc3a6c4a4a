"""One end-to-end pin of cvxpylayers_amd.cones.project against the layer: the projection of v in R^4 onto SOC(4) posed as the cone program
    min t  s.t.  (t, x - v) in SOC(5),  x in SOC(4),
solved and differentiated by the engine (v enters through b), must agree with the closed-form operation and its derivative within the parity gate of
BASELINE.md section 3 (1e-6 (1 + ||x||) on the solution, 1e-5 relative on the gradient)."""
import numpy as np
import pytest
import torch

from cvxpylayers_amd import cones as CN, problems as P
import cone_proj_kit as K

pytestmark = pytest.mark.gpu


def test_projection_onto_a_second_order_cone_as_a_layer():
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, _CvxpyLayer
    dev = torch.device("cuda", 0)
    B, n = 8, 5
    cones = {"z": 0, "l": 0, "q": [5, 4]}
    # solver form A u + s = b, u = (t, x):  s_1 = (t, x - v) = b_1 - A_1 u with A_1 = -I, b_1 = (0, -v);  s_2 = x with A_2 = [0 | -I], b_2 = 0
    A = np.zeros((9, n)); A[:5] = -np.eye(5); A[5:, 1:] = -np.eye(4)
    pattern = A != 0
    b_pattern = np.zeros(9, dtype=bool); b_pattern[1:5] = True
    tpl = P.dense_template(n, cones, pattern=pattern, b_pattern=b_pattern)
    c = np.zeros((B, n)); c[:, 0] = 1.0
    rng = np.random.default_rng(0)
    z = rng.standard_normal((B, 3))
    v = np.concatenate([(np.asarray(K.RHOS)[np.arange(B) % 4] * np.linalg.norm(z, axis=1))[:, None], z], axis=1)       # t = rho ||z||, the four rho twice
    A_eval0, q_eval = tpl.values_from_dense(np.broadcast_to(A, (B, 9, n)), np.zeros((B, 9)), c)
    A0, q_t = torch.from_numpy(A_eval0).to(dev), torch.from_numpy(q_eval).to(dev)
    assert list(tpl.b_idx) == [1, 2, 3, 4]                                   # b's structural entries: the rows that hold -v
    b_pos = torch.arange(int(tpl.indptr[-2]), int(tpl.indptr[-1]), device=dev)              # their positions in the value order
    w = torch.from_numpy(rng.standard_normal((B, 4))).to(dev)

    v_layer = torch.from_numpy(v).to(dev).requires_grad_(True)
    A_eval = A0.index_copy(0, b_pos, -v_layer.t())
    ctx = MI355_ctx(None, tpl.problem_data_index, cones, options={})
    primal, _, info, _ = _CvxpyLayer.apply(None, q_t, A_eval, ctx, {"eps": 1e-8, "acceleration_lookback": 0}, True, None)
    x_layer = primal[:, 1:]
    (g_layer,) = torch.autograd.grad((w * x_layer).sum(), v_layer)

    v_op = torch.from_numpy(v).to(dev).requires_grad_(True)
    x_op = CN.project(v_op, {"q": [4]})
    (g_op,) = torch.autograd.grad((w * x_op).sum(), v_op)

    xl, xo, gl, go = (t.detach().cpu().numpy() for t in (x_layer, x_op, g_layer, g_op))
    print("layer vs project: x", np.abs(xl - xo).max(), " gradient", np.abs(gl - go).max())
    assert (np.abs(xl - xo).max(axis=1) <= 1e-6 * (1 + np.linalg.norm(xo, axis=1))).all()
    assert (np.linalg.norm(gl - go, axis=1) <= 1e-5 * np.maximum(np.linalg.norm(go, axis=1), np.linalg.norm(w.cpu().numpy(), axis=1))).all()
