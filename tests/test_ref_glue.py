"""The repository's boundary glue pinned on what the REFERENCE's own glue returned (CPU; runs anywhere).

tests/golden/make_refglue.py runs the reference's frontend (torch/cvxpylayer.py) and DIFFCP plugin (interfaces/diffcp_if.py) unchanged,
with cvxpy stubbed (canonicalisation is bypassed: hand-canonicalised templates) and diffcp's two calls served by the CPU oracle, and
records what they return: tests/golden/refglue_<case>.npz (whole forward + backward of the seeded cases of tests/ref_cases.py) and
tests/golden/refglue_conventions.npz (the boundary functions on the seeded inputs of ref_cases.py).  `make_refglue.py --check`
re-runs the reference against these files and applies the INTEGRATION.md hunks to its sources.  Checked here, against the records:
  * the repository's glue (frontend flattening and maps, the plugin convention served by the oracle, variable recovery, the
    backward through the maps) reproduces every tensor of the recorded runs, link by link;
  * the recorded runs reproduce the closed forms the reference's tests assert (values and gradients), i.e. reference glue + oracle
    is a faithful stand-in for reference glue + diffcp on these problems;
  * the repository's restated conventions equal what the reference functions returned: (A, b, c) cut out of A_eval / q_eval
    (_build_diffcp_matrices), gradient packing (_compute_gradients), parameter flattening + column order
    (_flatten_and_batch_params vs the frontend's row-major re-indexed maps), variable recovery (_recover_results), error
    messages of validate_params, solver_args merging.
"""
import os
import sys

import numpy as np
import pytest
import torch

import ref_cases

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_refglue import norm_message  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def conv():
    return np.load(os.path.join(GOLD, "refglue_conventions.npz"))


def _repo_layer(template):
    from cvxpylayers_amd.torch import CvxpyLayer
    return CvxpyLayer(template=template)


@pytest.mark.parametrize("name", list(ref_cases.CASES))
def test_fixtures_are_outputs_of_the_reference_glue(name):
    """Replays a recorded run of the reference glue link by link through this repository's glue: parameters -> (frontend flattening,
    maps) -> A_eval / q_eval -> (plugin convention, oracle) -> primal / dual -> (recovery) -> outputs; and backward: d primal / d dual ->
    dA_eval / dq_eval -> (maps transposed, un-flattening) -> parameter gradients.  Each link starts from the recorded input."""
    from oracle_layer import OraclePlugin
    case = ref_cases.CASES[name]()
    tpl = case["template"]
    want = np.load(os.path.join(GOLD, f"refglue_{name}.npz"))
    close = lambda got, k: np.testing.assert_allclose(got, want[k], rtol=1e-9, atol=1e-11, err_msg=f"{name}:{k}")
    nparams = len(case["params"])
    assert sorted(want.files) == sorted([f"{p}{k}" for k in range(nparams) for p in ("param", "grad")] +
                                        [f"{p}{k}" for k in range(len(case["weights"])) for p in ("out", "weight")] +
                                        [p + t for t in ("q_eval", "A_eval", "primal", "dual") for p in ("", "d")])
    for k in range(nparams):
        np.testing.assert_array_equal(want[f"param{k}"], np.asarray(case["params"][k], dtype=np.float64))
    for k, w in enumerate(case["weights"]):
        np.testing.assert_array_equal(want[f"weight{k}"], np.asarray(w))
    B = want["primal"].shape[0]
    bm = lambda k: torch.tensor(want[k].reshape(-1, B))                     # (rows, B): an unbatched run records 1-D boundary tensors
    # parameters -> A_eval / q_eval, and back
    mine = _repo_layer(tpl)
    params = [torch.tensor(want[f"param{k}"], requires_grad=True) for k in range(nparams)]
    batch = mine.validate_params(list(params))
    p_bm = mine._flatten_params(params, batch)
    A_bm = p_bm @ torch.tensor(mine._A.mat.toarray()).t(); q_bm = p_bm @ torch.tensor(mine._q.mat.toarray()).t()
    np.testing.assert_allclose(A_bm.t().detach().numpy(), bm("A_eval").numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(q_bm.t().detach().numpy(), bm("q_eval").numpy(), rtol=0, atol=1e-13)
    torch.autograd.backward([A_bm.t(), q_bm.t()], [bm("dA_eval"), bm("dq_eval")])
    for k, p in enumerate(params):
        close(p.grad.numpy(), f"grad{k}")
    # the plugin convention served by the oracle: primal / dual and, from the recorded cotangents, dA_eval / dq_eval
    q_eval = bm("q_eval").requires_grad_(); A_eval = bm("A_eval").requires_grad_()
    primal, dual, _, _ = OraclePlugin.apply(None, q_eval, A_eval, tpl, {**ref_cases.SOLVER_ARGS, "mode": "dense"}, True, None)
    close(primal.detach().numpy(), "primal"); close(dual.detach().numpy(), "dual")
    torch.autograd.backward([primal, dual], [torch.tensor(want["dprimal"]), torch.tensor(want["ddual"])])
    close(A_eval.grad.numpy().reshape(want["dA_eval"].shape), "dA_eval"); close(q_eval.grad.numpy().reshape(want["dq_eval"].shape), "dq_eval")
    # recovery, and the cotangents the loss hands back to the plugin
    pr = torch.tensor(want["primal"], requires_grad=True); du = torch.tensor(want["dual"], requires_grad=True)
    outs = mine._recover_results_torch(pr, du, batch)
    assert len(outs) == len(case["weights"])
    for k, o in enumerate(outs):
        close(o.detach().numpy(), f"out{k}")
    sum((o * torch.tensor(want[f"weight{k}"])).sum() for k, o in enumerate(outs)).backward()
    for t, k in ((pr, "dprimal"), (du, "ddual")):                          # no output read from it: the recorder stored zeros
        close((t.grad if t.grad is not None else torch.zeros_like(t)).numpy(), k)


def test_reference_glue_plus_oracle_reproduces_the_reference_tests_closed_forms():
    # tests/test_torch.py:90-118 (ridge value + gradient, atol 1e-6 at eps 1e-10) through the reference's own frontend + plugin
    f = np.load(os.path.join(GOLD, "refglue_ridge_batched_matrix_param.npz"))
    F = torch.tensor(f["param0"], requires_grad=True); g = torch.tensor(f["param1"], requires_grad=True)
    n = F.shape[2]
    x = torch.linalg.solve(F.transpose(1, 2) @ F + torch.eye(n, dtype=torch.float64), (F.transpose(1, 2) @ g[:, :, None]))[:, :, 0]
    (x * torch.tensor(f["weight0"])).sum().backward()
    np.testing.assert_allclose(f["out0"], x.detach().numpy(), atol=1e-6)
    np.testing.assert_allclose(f["grad0"], F.grad.numpy(), atol=1e-6)
    np.testing.assert_allclose(f["grad1"], g.grad.numpy(), atol=1e-6)
    # broadcast parameter: the gradient is the SUM over the batch (tests/test_torch.py:355-384)
    f = np.load(os.path.join(GOLD, "refglue_ridge_mixed.npz"))
    F = torch.tensor(f["param0"], requires_grad=True); g = torch.tensor(f["param1"], requires_grad=True)
    x = torch.linalg.solve(F.t() @ F + torch.eye(F.shape[1], dtype=torch.float64), F.t() @ g.t()).t()
    (x * torch.tensor(f["weight0"])).sum().backward()
    np.testing.assert_allclose(f["out0"], x.detach().numpy(), atol=1e-6)
    np.testing.assert_allclose(f["grad0"], F.grad.numpy(), atol=1e-6)
    # SDP: X = v v^T, PSD dual = C - lmin I (tests/test_dual_variables.py:523-550), gradient through eigh (tests/test_torch.py:233-248)
    f = np.load(os.path.join(GOLD, "refglue_sdp_sym_primal_psd_dual.npz"))
    C = torch.tensor(f["param0"], requires_grad=True)
    w, V = torch.linalg.eigh(0.5 * (C + C.transpose(1, 2)))
    X = V[:, :, 0, None] * V[:, None, :, 0]
    Z = 0.5 * (C + C.transpose(1, 2)) - w[:, 0, None, None] * torch.eye(C.shape[1], dtype=torch.float64)
    ((X * torch.tensor(f["weight0"])).sum() + (Z * torch.tensor(f["weight1"])).sum()).backward()
    np.testing.assert_allclose(f["out0"], X.detach().numpy(), atol=1e-6)
    np.testing.assert_allclose(f["out1"], Z.detach().numpy(), atol=1e-6)
    np.testing.assert_allclose(f["grad0"], C.grad.numpy(), atol=1e-5)


def test_build_diffcp_matrices_is_what_the_restated_conventions_say(conv):
    """diffcp_if.py:46-70 on seeded boundary values (recorded) vs cvxpylayers_amd.problems.ConeTemplate.dense_from_values (the
    convention every oracle comparison in this repository goes through): A = -A_aug[:, :-1], b = A_aug[:, -1], c = q[:-1]."""
    d = ref_cases.diffcp_matrices_inputs()
    tpl, n, B = d["tpl"], d["n"], d["B"]
    A, b, c = tpl.dense_from_values(d["A_eval"], d["q_eval"])
    for i in range(B):
        np.testing.assert_array_equal(conv[f"bdm_A{i}"], A[i]); np.testing.assert_array_equal(conv[f"bdm_b{i}"], b[i]); np.testing.assert_array_equal(conv[f"bdm_c{i}"], c[i])
        np.testing.assert_array_equal(conv[f"bdm_bidx{i}"], tpl.b_idx)
    # _compute_gradients (:73-96) with a known adjoint: dA_eval = [-dA.data (CSC order of A), db[b_idx]], dq_eval = [dc, 0]
    cols_aug = np.repeat(np.arange(n + 1), np.diff(tpl.indptr))
    for i in range(B):
        aug = np.concatenate([-d["dA"][i], d["db"][i][:, None]], axis=1)       # d/d[A_cvx | b_cvx] with A = -A_cvx
        np.testing.assert_allclose(conv[f"bdm_dA{i}"], aug[tpl.indices, cols_aug])
        np.testing.assert_allclose(conv[f"bdm_dq{i}"], np.concatenate([d["dc"][i], [0.0]]))
    # and the repository's own packing (problems.ConeTemplate.values_from_dense) is the same
    dA_eval, dq_eval = tpl.values_from_dense(d["dA"], d["db"], d["dc"])
    for i in range(B):
        np.testing.assert_allclose(dA_eval[:, i], conv[f"bdm_dA{i}"]); np.testing.assert_allclose(dq_eval[:, i], conv[f"bdm_dq{i}"])


@pytest.mark.parametrize("name", ref_cases.FLATTENING_CASES)
def test_flattening_and_maps_agree_with_the_reference_frontend(conv, name):
    """reference: p_stack = _flatten_and_batch_params (Fortran, canonical column order, (Ptot+1, B)); A_eval = A_map @ p_stack.
    repository: p_bm (B, Ptot+1) row-major against maps whose columns were re-indexed once.  Same A_eval / q_eval."""
    case = ref_cases.CASES[name]()
    tpl = case["template"]
    params = [torch.tensor(np.asarray(p)) for p in case["params"]]
    p_stack = conv[f"flat_{name}_p_stack"]
    mine = _repo_layer(tpl)
    batch = mine.validate_params(list(params))
    assert tuple(batch) == tuple(conv[f"flat_{name}_batch"]) and tuple(mine.batch_sizes) == tuple(conv[f"flat_{name}_batch_sizes"])
    p_bm = mine._flatten_params(params, batch).numpy()
    np.testing.assert_allclose(mine._A.mat @ p_bm.T, tpl.A_map @ p_stack, rtol=0, atol=1e-13)
    np.testing.assert_allclose(mine._q.mat @ p_bm.T, tpl.q_map @ p_stack, rtol=0, atol=1e-13)
    f = np.load(os.path.join(GOLD, f"refglue_{name}.npz"))               # and these are the tensors the reference plugin received
    np.testing.assert_allclose(tpl.A_map @ p_stack, f["A_eval"], atol=1e-13)


@pytest.mark.parametrize("name", ref_cases.RECOVERY_CASES)
def test_variable_recovery_agrees_with_the_reference(conv, name):
    case = ref_cases.CASES[name]()
    tpl = case["template"]
    mine = _repo_layer(tpl)
    for batch, primal, dual in ref_cases.recovery_inputs(tpl):
        primal = torch.tensor(primal); dual = torch.tensor(dual)
        want = [conv[f"rec_{name}_{len(batch)}_{k}"] for k in range(int(conv[f"rec_{name}_{len(batch)}_count"]))]
        got = mine._recover_results_torch(primal, dual, batch)       # the per-variable chain (checker of the one-launch device path)
        assert len(want) == len(got)
        for a, b in zip(want, got):
            assert a.shape == tuple(b.shape) and np.array_equal(a, b.numpy())
        # the sparse recovery map the device path launches (ce_parammap_apply2), applied here with scipy: same numbers, same layout
        for source, src in (("primal", primal), ("dual", dual)):
            if source not in mine._rec:
                continue
            csr, layout = mine._rec[source]
            rec = (csr.mat @ src.numpy().T).T
            for pos, off, size in layout:
                w = want[pos]
                assert np.array_equal(rec[:, off:off + size].reshape(w.shape), w)


def test_validate_params_messages_are_the_references(conv):
    tpl = ref_cases.CASES["ridge_mixed"]()["template"]
    mine = _repo_layer(tpl)
    bad = ref_cases.bad_ridge_params(tpl)
    assert len(conv["validate_messages"]) == len(bad)
    for vals, want in zip(bad, conv["validate_messages"]):
        with pytest.raises(ValueError) as e_mine:
            mine.validate_params(list(vals))
        assert norm_message(e_mine.value) == str(want)


def test_solver_args_reach_diffcp_merged_and_unmutated(conv):
    """diffcp_if.py:356-359: merged = {**ctx.options, **solver_args}; neither dict is mutated (tests/test_parse_args.py:224-248)."""
    layer_opts, call = ref_cases.SOLVER_ARGS_LAYER, ref_cases.SOLVER_ARGS_CALL
    assert str(conv["solver_args_call"]) == "solve_only_batch"                                      # no grad needed -> solve_only_batch
    assert float(conv["solver_args_eps"]) == call["eps"] and int(conv["solver_args_max_iters"]) == layer_opts["max_iters"]
    assert bool(conv["solver_args_unmutated"])
    # the repository's plugin merges the same way
    from cvxpylayers_amd.interfaces.mi355_if import make_settings
    lo, ca = dict(layer_opts), dict(call)
    s = make_settings({**lo, **ca})
    assert s.eps_abs == 1e-9 and s.max_iters == 1234
    assert lo == layer_opts and ca == call
