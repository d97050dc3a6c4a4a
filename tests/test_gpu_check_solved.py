"""k_check_solved (include/cone_engine.h ce_check_solved; csrc/ce_check.h) against the numpy float64 statement of the forward kernels' termination test
(newton_first_kit.termination_test).

Shapes: n = 3 with a row that has no b slot; n = 12 mixed cones (m = 19: rows and columns share workgroup passes unevenly); n = 9 with an exponential and a power
triple; the native box QP with its one-triangle P structure and with a full symmetric one.  B = 1, 5, 67 (one workgroup per instance; the counting kernel sums over the batch), A batch-major and batch-minor, q in both stride orders.
Points of a batch, by position i % 10: oracle solutions at eps = 1e-10 (0, 5, 8), at eps = 1e-3 (1, 6), an ineligible instance that would pass (2), a NaN in x
(3), and planted single failures -- one b entry shifted on a row with y_r = 0: primal only (4); one c entry shifted on a column where x_j = 0: dual only (7);
b_r and s_r shifted together on a row with y_r != 0: gap only (9).  Every batch is tested at eps = 1e-6 and at eps = 1e-8.
Bounds: decisions equal numpy's, every comparison at least 1e-9 (relative) away from its threshold so that rounding cannot flip it; resid within
1e-12 (1 + sum |terms of the row|) of numpy; untouched outputs keep a sentinel; n_unsolved exact; instance 0 alone bit-equal to instance 0 of the batch of 67."""
import numpy as np
import pytest
import torch

from cvxpylayers_amd import problems as P
from newton_first_kit import margins, termination_test
from oracle import oracle
from qp_ns_kit import full_structure
from test_quad_objective import _p_values

BMAX = 67
SHIFT = 1e-2
TEMPLATES = ("no_b_slot", "small", "triples", "qp_tri", "qp_full")
_CACHE = {}


def _case(name):
    """(tpl, cones, A, b, c, Pm, struct, tight, loose) for BMAX instances, solved once per module"""
    if name in _CACHE:
        return _CACHE[name]
    Pm = struct = None
    if name == "no_b_slot":
        n, cones = 3, {"z": 1, "l": 3, "q": []}
        b_pattern = np.array([True, True, False, True])
        tpl = P.dense_template(n, cones, b_pattern=b_pattern)
        A, b, c = P.generate(n, cones, BMAX, seed=2)
        b = b * b_pattern[None]
    elif name == "small":
        n, cones = 12, {"z": 2, "l": 8, "q": [4, 5]}
        tpl = P.dense_template(n, cones)
        A, b, c = P.generate(n, cones, BMAX, seed=1)
    elif name == "triples":
        n, cones = 9, {"z": 1, "l": 5, "q": [3], "s": [], "ep": 1, "p": [0.4]}
        tpl = P.dense_template(n, cones)
        A, b, c = P.generate(n, cones, BMAX, seed=3)
    else:
        nx = 10
        A0, b, c, P0, pst, _ = P.native_box_qp_batch(nx, BMAX, seed=2)
        cones = {"z": 0, "l": 2 * nx, "q": []}
        A = np.broadcast_to(A0, (BMAX,) + A0.shape).copy()
        Pm = np.broadcast_to(P0, (BMAX, nx, nx)).copy() * (1 + 0.1 * np.random.default_rng(7).random((BMAX, 1, 1)))
        struct = pst if name == "qp_tri" else full_structure(nx)
        tpl = P.dense_template(nx, cones, pattern=(A0 != 0))
    tight = oracle.solve_batch(A, b, c, cones, P=Pm, eps=1e-10, max_iters=200000)
    loose = oracle.solve_batch(A, b, c, cones, P=Pm, eps=1e-3)
    # (a tiny instance may be solved to 1e-8 by the time the oracle's 1e-3 test first looks: such a point is no loose point, the instance keeps its tight one)
    loose["is_loose"] = ~termination_test(A, b, c, loose["x"], loose["y"], loose["s"], 1e-8, 1e-8, Pm=Pm)["solved"]
    _CACHE[name] = (tpl, cones, A, b, c, Pm, struct, tight, loose)
    return _CACHE[name]


def _batch(name, B):
    """data and points of the first B instances with the roles of the module docstring; a role that cannot be planted on an instance leaves it a tight solution"""
    tpl, cones, A, b, c, Pm, struct, tight, loose = _case(name)
    A, b, c = A[:B].copy(), b[:B].copy(), c[:B].copy()
    Pm = Pm[:B].copy() if Pm is not None else None
    x, y, s = (tight[k][:B].copy() for k in ("x", "y", "s"))
    eligible = np.ones(B, np.int32)
    b_slot = np.zeros(tpl.m, bool); b_slot[tpl.b_idx] = True
    roles = []
    for i in range(B):
        role = ("tight", "loose", "ineligible", "nan", "primal", "tight", "loose", "dual", "tight", "gap")[i % 10]
        if role == "loose" and not loose["is_loose"][i]:
            role = "tight"
        if role == "loose":
            x[i], y[i], s[i] = loose["x"][i], loose["y"][i], loose["s"][i]
        elif role == "ineligible":
            eligible[i] = 2          # (some other bit of the word: the mask decides)
        elif role == "nan":
            x[i, i % tpl.n] = np.nan
        elif role == "primal":
            rows = np.nonzero((y[i] == 0) & b_slot)[0]
            if len(rows):
                b[i, rows[0]] += SHIFT
            else:
                role = "tight"
        elif role == "dual":
            if Pm is None:          # x_j := 0 with b moved along column j keeps A x + s = b and leaves A^T y + c alone; then c_j moves the dual residual only
                j = i % tpl.n
                if b_slot.all() or not (A[i, ~b_slot, j] != 0).any():
                    b[i] -= A[i, :, j] * x[i, j]; x[i, j] = 0.0; c[i, j] += SHIFT
                else:
                    role = "tight"
            else:
                role = "tight"
        elif role == "gap":
            rows = np.nonzero((np.abs(y[i]) > 1e-2) & b_slot)[0]
            if len(rows):
                b[i, rows[0]] += SHIFT; s[i, rows[0]] += SHIFT
            else:
                role = "tight"
        roles.append(role)
    return tpl, A, b, c, Pm, struct, x, y, s, eligible, roles


def _engine(tpl):
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    key = ("eng", id(tpl))
    if key not in _CACHE:
        _CACHE[key] = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0))
    return _CACHE[key]


def _run(name, B, layout, eps):
    tpl, A, b, c, Pm, struct, x, y, s, eligible, roles = _batch(name, B)
    eng = _engine(tpl)
    dev = eng.device
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    if layout == "batch_major":
        A_t = torch.from_numpy(np.ascontiguousarray(A_eval.T)).to(dev).t(); q_t = torch.from_numpy(np.ascontiguousarray(q_eval.T)).to(dev).t()
    else:
        A_t = torch.from_numpy(np.ascontiguousarray(A_eval)).to(dev); q_t = torch.from_numpy(np.ascontiguousarray(q_eval)).to(dev)
    P_bm = p_struct = None
    if Pm is not None:
        P_bm = torch.from_numpy(np.ascontiguousarray(_p_values(Pm, struct))).to(dev)
        cols = np.repeat(np.arange(tpl.n), np.diff(struct[1])).astype(np.int32)
        p_struct = (torch.from_numpy(np.ascontiguousarray(struct[0], dtype=np.int32)).to(dev), torch.from_numpy(cols).to(dev))
    status = torch.full((B,), -77, dtype=torch.int32, device=dev); iters = torch.full((B,), -5, dtype=torch.int32, device=dev)
    resid = torch.full((B, 3), -3.0, dtype=torch.float64, device=dev)
    solved, status, iters, resid, n_uns = eng.check_solved(A_t, q_t, *(torch.from_numpy(t).to(dev) for t in (x, y, s)), eps, eps,
                                                           eligible=torch.from_numpy(eligible).to(dev), eligible_mask=1, P_bm=P_bm, p_structure=p_struct,
                                                           status=status, iters=iters, resid=resid)
    torch.cuda.synchronize()
    want = termination_test(A, b, c, x, y, s, eps, eps, Pm=Pm, eligible=eligible & 1)
    would = termination_test(A, b, c, x, y, s, eps, eps, Pm=Pm)
    return dict(solved=solved.cpu().numpy().astype(bool), status=status.cpu().numpy(), iters=iters.cpu().numpy(), resid=resid.cpu().numpy(),
                n_unsolved=int(n_uns.cpu()[0]), want=want, would=would, roles=roles)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["batch_major", "batch_minor"])
@pytest.mark.parametrize("B", [1, 5, BMAX])
@pytest.mark.parametrize("name", TEMPLATES)
def test_decisions_residuals_and_untouched_outputs_match_numpy(name, B, layout):
    for eps in (1e-6, 1e-8):
        r = _run(name, B, layout, eps)
        want, roles = r["want"], np.array(r["roles"])
        mg = margins(want)
        print(f"{name} B={B} {layout} eps={eps:g}: solved {int(r['solved'].sum())} (numpy {int(want['solved'].sum())}), smallest margin {mg.min():.2e}")
        assert mg.min() >= 1e-9, "a comparison of the reference sits within rounding of its threshold: the case decides nothing"
        if eps == 1e-6:
            assert want["solved"][roles == "tight"].all()
        else:
            assert not want["solved"][roles == "loose"].any()
        assert not want["solved"][(roles == "ineligible") | (roles == "nan")].any()
        if eps == 1e-6:
            assert r["would"]["solved"][roles == "ineligible"].all(), "the ineligible instance must be one that would pass"
        np.testing.assert_array_equal(r["solved"], want["solved"])
        assert r["n_unsolved"] == int((~want["solved"]).sum())
        ok = want["solved"]
        err = np.abs(r["resid"][ok] - want["resid"][ok]); bound = 1e-12 * (1 + want["terms"][ok])
        if ok.any():
            print(f"    max |resid - numpy| / bound = {(err / bound).max():.3e}")
        assert (err <= bound).all()
        assert (r["status"][ok] == 1).all() and (r["iters"][ok] == 0).all()
        assert (r["status"][~ok] == -77).all() and (r["iters"][~ok] == -5).all() and (r["resid"][~ok] == -3.0).all()


@pytest.mark.gpu
def test_each_inequality_is_the_only_failing_one_somewhere():
    r = _run("small", BMAX, "batch_major", 1e-6)
    passed, roles = r["want"]["passed"], np.array(r["roles"])
    for role, col in (("primal", 0), ("dual", 1), ("gap", 2)):
        only = [list(p) == [k != col for k in range(3)] for p in passed[roles == role]]
        assert len(only) and all(only), (role, passed[roles == role])
    np.testing.assert_array_equal(r["solved"], r["want"]["solved"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", TEMPLATES)
def test_an_instance_alone_is_bit_equal_to_itself_inside_the_batch(name):
    one, many = _run(name, 1, "batch_major", 1e-6), _run(name, BMAX, "batch_major", 1e-6)
    assert one["solved"][0] and many["solved"][0]
    np.testing.assert_array_equal(one["resid"][0], many["resid"][0])
