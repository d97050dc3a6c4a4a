"""Generates tests/golden/refglue_<case>.npz by running the REFERENCE's own frontend + DIFFCP plugin code (tests/ref_glue.py:
the reference's sources executed unchanged, cvxpy / diffcp stubbed, diffcp's arithmetic done by the CPU oracle) on the seeded cases
of tests/ref_cases.py, and tests/golden/refglue_conventions.npz with what the reference's boundary functions return for the seeded
inputs of ref_cases.py (matrix building, gradient packing, flattening, variable recovery, error messages, solver_args merging).
Needs a checkout of the reference (see tests/ref_glue.py).

    python tests/golden/make_refglue.py            # write the fixtures
    python tests/golden/make_refglue.py --check    # re-run the reference and compare with the committed fixtures; apply the
                                                   # INTEGRATION.md hunks to the reference's sources and check the routing

Each refglue_<case>.npz holds: the parameters, the layer outputs and the parameter gradients of loss = sum_k <out_k, weight_k>, and the
tensors that crossed the plugin boundary in that run (q_eval, A_eval, primal, dual and their gradients)."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_cases  # noqa: E402
import ref_glue  # noqa: E402


def norm_message(s):
    """validate_params messages with torch.Size([a, b]) written as (a, b): the form both sides are compared in"""
    return re.sub(r"torch\.Size\(\[([^\]]*)\]\)", r"(\1)", str(s)).replace(",)", ")")


def record_conventions(ns):
    """What the reference's boundary functions return for the seeded inputs of ref_cases.py: {name: array}."""
    import torch
    out = {}
    # diffcp_if._build_diffcp_matrices / _compute_gradients
    d = ref_cases.diffcp_matrices_inputs()
    tpl, n, B = d["tpl"], d["n"], d["B"]
    As, bs, cs, b_idxs = ns.diffcp_if._build_diffcp_matrices(torch.tensor(d["A_eval"]), torch.tensor(d["q_eval"]), (tpl.indices, tpl.indptr), (tpl.m, n + 1), tpl.b_idx, B)

    def adj(dxs, dys, dss):
        assert all(np.all(v == 0) for v in dss)                       # ds = 0 (diffcp_if.py:84)
        res = []
        for i in range(B):
            cols = np.repeat(np.arange(n), np.diff(As[i].indptr))
            res.append(type(As[i])((d["dA"][i][As[i].indices, cols], As[i].indices, As[i].indptr), shape=As[i].shape))
        return res, list(d["db"]), list(d["dc"])
    dq_b, dA_b = ns.diffcp_if._compute_gradients(adj, np.zeros((B, n)), np.zeros((B, tpl.m)), bs, b_idxs, B)
    for i in range(B):
        out[f"bdm_A{i}"] = As[i].toarray(); out[f"bdm_b{i}"] = np.asarray(bs[i]); out[f"bdm_c{i}"] = np.asarray(cs[i])
        out[f"bdm_bidx{i}"] = np.asarray(b_idxs[i]); out[f"bdm_dq{i}"] = np.asarray(dq_b[i]); out[f"bdm_dA{i}"] = np.asarray(dA_b[i])
    # cvxpylayer._flatten_and_batch_params, validate_params' batch
    for name in ref_cases.FLATTENING_CASES:
        case = ref_cases.CASES[name]()
        rl = ref_glue.reference_layer(ns, case["template"])
        params = [torch.tensor(np.asarray(p)) for p in case["params"]]
        batch = rl.ctx.validate_params(list(params))
        out[f"flat_{name}_p_stack"] = ns.cvxpylayer._flatten_and_batch_params(tuple(params), rl.ctx, batch).numpy()
        out[f"flat_{name}_batch"] = np.asarray(batch, dtype=np.int64)
        out[f"flat_{name}_batch_sizes"] = np.asarray(rl.ctx.batch_sizes, dtype=np.int64)
    # cvxpylayer._recover_results
    for name in ref_cases.RECOVERY_CASES:
        tpl = ref_cases.CASES[name]()["template"]
        rl = ref_glue.reference_layer(ns, tpl)
        for batch, primal, dual in ref_cases.recovery_inputs(tpl):
            want = ns.cvxpylayer._recover_results(torch.tensor(primal), torch.tensor(dual), rl.ctx, batch)
            out[f"rec_{name}_{len(batch)}_count"] = np.asarray(len(want))
            for k, w in enumerate(want):
                out[f"rec_{name}_{len(batch)}_{k}"] = w.numpy()
    # LayersContext.validate_params error messages
    tpl = ref_cases.CASES["ridge_mixed"]()["template"]
    rl = ref_glue.reference_layer(ns, tpl)
    msgs = []
    for vals in ref_cases.bad_ridge_params(tpl):
        try:
            rl.ctx.validate_params(list(vals))
        except ValueError as e:
            msgs.append(norm_message(e))
        else:
            raise AssertionError(f"the reference accepted {[tuple(v.shape) for v in vals]}")
    out["validate_messages"] = np.asarray(msgs)
    # solver_args: layer-level merged with call-level, neither dict mutated (diffcp_if.py:356-359)
    case = ref_cases.CASES["ridge_unbatched"]()
    layer_opts, call = dict(ref_cases.SOLVER_ARGS_LAYER), dict(ref_cases.SOLVER_ARGS_CALL)
    rl = ref_glue.reference_layer(ns, case["template"], solver_args=layer_opts)
    ns.diffcp.calls.clear()
    rl(*[torch.tensor(np.asarray(p)) for p in case["params"]], solver_args=call)
    fn, kw = ns.diffcp.calls[-1]
    out["solver_args_call"] = np.asarray(fn)
    out["solver_args_eps"] = np.asarray(float(kw["eps"])); out["solver_args_max_iters"] = np.asarray(int(kw["max_iters"]))
    out["solver_args_unmutated"] = np.asarray(layer_opts == ref_cases.SOLVER_ARGS_LAYER and call == ref_cases.SOLVER_ARGS_CALL)
    return out


def check_integration_hunks(ns):
    """the hunks (tests/integration_hunks.py holds them in machine-applicable form) applied to the reference's
    source text in memory; the patched registry returns this repository's context / plugin for solver="MI355", and the patched reference
    frontend reaches the plugin and hands it warm_start (which the unpatched frontend refuses for every solver but MOREAU)."""
    import torch
    import integration_hunks as ih
    from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, _CvxpyLayer
    with ih.patched_reference_modules(ns) as patched:
        assert patched.interfaces.get_torch_cvxpylayer("MI355") is _CvxpyLayer
        assert patched.interfaces.get_torch_cvxpylayer("DIFFCP") is ns.diffcp_if._CvxpyLayer
        case = ref_cases.CASES["ridge_unbatched"]()
        layer = ref_glue.reference_layer(patched, case["template"], solver="MI355", solver_args={"eps": 1e-8})
        assert isinstance(layer.ctx.solver_ctx, MI355_ctx) and layer.ctx.solver_ctx.options == {"eps": 1e-8}
        params = [torch.tensor(np.asarray(p), requires_grad=True) for p in case["params"]]
        try:
            ref_glue.reference_layer(ns, case["template"])(*params, warm_start=True)
            raise AssertionError("the unpatched reference frontend accepted warm_start for DIFFCP")
        except ValueError as e:
            assert "only supported" in str(e)
        seen = {}

        class Spy:
            @staticmethod
            def apply(P_eval, q_eval, A_eval, cl_ctx, solver_args, needs_grad, warm_start):
                seen["ws"] = warm_start
                raise KeyboardInterrupt
        orig = patched.interfaces.get_torch_cvxpylayer
        patched.interfaces.get_torch_cvxpylayer = lambda s: Spy
        try:
            layer(*params, warm_start=True)
        except KeyboardInterrupt:
            pass
        finally:
            patched.interfaces.get_torch_cvxpylayer = orig
        assert seen["ws"] is True


def _compare(name, got, want):
    assert sorted(got) == sorted(want.files), name
    for k in want.files:
        if got[k].dtype.kind in "US" or want[k].dtype.kind in "US":
            assert np.array_equal(got[k], want[k]), f"{name}:{k}"
        else:
            np.testing.assert_allclose(got[k], want[k], rtol=1e-9, atol=1e-11, err_msg=f"{name}:{k}")


if __name__ == "__main__":
    check = "--check" in sys.argv[1:]
    args = {**ref_cases.SOLVER_ARGS, "mode": "dense"}
    with ref_glue.reference_modules() as ns:
        for name, make in ref_cases.CASES.items():
            out = ref_glue.run_case(ns, make(), args)
            path = os.path.join(HERE, f"refglue_{name}.npz")
            if check:
                _compare(name, out, np.load(path))
            else:
                np.savez_compressed(path, **out)
            print(name, {k: v.shape for k, v in out.items() if k.startswith(("out", "grad"))})
        out = record_conventions(ns)
        path = os.path.join(HERE, "refglue_conventions.npz")
        if check:
            _compare("conventions", out, np.load(path))
            check_integration_hunks(ns)
            print("fixtures and integration hunks: ok")
        else:
            np.savez_compressed(path, **out)
            print("conventions", len(out), "arrays")
