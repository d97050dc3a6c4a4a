"""Time of the forward derivative and of one Newton refinement step with the quadratic objective inside the kernels (ce_jvp_qp, ce_refine_qp: k_backward_ns<..., QP>)
next to the adjoint of the same template (ce_vjp_qp: the pivoting kernel k_backward_rt, the yardstick) at configuration 2 in its native form (box QP, n = 50, 100
bound rows): same shape, same eps point, same process.  Protocol of scripts/jvp_direct_timing.py: events on the launch stream around each call, warm-up calls first,
then --reps timed calls each, the three interleaved so that clock drift hits all.  The refinement step runs on a clone of the point, made outside the events.
Prints one JSON line (mean, median, min, max in ms; flagged shares; ratios); --out also writes it to a file.

    python scripts/jvp_qp_timing.py [--B 4096] [--reps 20] [--warmup 5] [--eps 1e-8] [--out profiles/jvp/jvp_qp_direct_C2.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cvxpylayers_amd import _lib  # noqa: E402
from cvxpylayers_amd import problems as P  # noqa: E402
from cvxpylayers_amd.interfaces.mi355_if import ConeEngine, make_settings  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=P.CONFIGS["C2"]["B"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eps", type=float, default=1e-8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    nx, B = 50, a.B
    # the native box QP of BASELINE configuration 2, per-instance P (tests/test_quad_objective.py::test_native_qp_kernels_match_the_oracle_on_box_qps)
    rng = np.random.default_rng(0)
    Fm = rng.standard_normal((nx, nx)) / np.sqrt(nx); g = rng.standard_normal((B, nx))
    lo = -0.5 - 0.5 * rng.random((B, nx)); hi = 0.5 + 0.5 * rng.random((B, nx))
    Pn = np.broadcast_to(2 * Fm.T @ Fm, (B, nx, nx)) * (1 + 0.1 * rng.random((B, 1, 1)))
    An = np.broadcast_to(np.concatenate([-np.eye(nx), np.eye(nx)], axis=0), (B, 2 * nx, nx))
    cones = {"z": 0, "l": 2 * nx, "q": []}
    tpl = P.dense_template(nx, cones, pattern=(An[0] != 0))
    rows, ptr = [], [0]
    for j in range(nx):
        rows.extend(range(j + 1)); ptr.append(len(rows))
    idx, ptr = np.asarray(rows, dtype=np.int32), np.asarray(ptr, dtype=np.int32)          # upper triangle, CSC
    eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, cones, torch.device("cuda", 0), p_structure=(idx, ptr))
    assert eng.qp_native
    A_eval, q_eval = tpl.values_from_dense(An, np.concatenate([-lo, hi], axis=1), -2 * g @ Fm)
    A_bm = torch.from_numpy(A_eval).cuda().t().contiguous(); q_t = torch.from_numpy(q_eval).cuda()
    P_bm = torch.from_numpy(np.ascontiguousarray(Pn[:, idx, np.repeat(np.arange(nx), np.diff(ptr))])).cuda()
    x, y, s, _, status, _ = eng.solve(A_bm, q_t, make_settings(dict(eps=a.eps, acceleration_lookback=0, max_iters=100000)), P_bm=P_bm)
    assert (status == 1).all()
    xb = torch.from_numpy(rng.standard_normal((B, tpl.n))).cuda(); yb = torch.zeros((B, tpl.m), dtype=torch.float64, device="cuda")
    tA = torch.from_numpy(rng.standard_normal((B, tpl.nnz_aug))).cuda(); tq = torch.from_numpy(rng.standard_normal((tpl.n + 1, B))).cuda()
    tP = torch.from_numpy(rng.standard_normal((B, eng.nnz_p))).cuda()
    last = {}
    pt = {}

    def jvp_qp():
        last["jvp_qp"] = eng.jvp(A_bm, x, y, s, tA, tq, method="direct", P_bm=P_bm, tP_bm=tP)[3]
        assert eng.last_jvp_kernel == "ce_jvp_qp"

    def refine_qp():
        last["refine_qp"] = eng.refine(A_bm, q_t, *pt["clone"], 1, status=status, P_bm=P_bm)[3]["status"]

    def vjp_qp():
        last["vjp_qp"] = eng.vjp(A_bm, x, y, s, xb, yb, P_bm=P_bm)[2]
    calls = (("jvp_qp", jvp_qp), ("refine_qp_one_step", refine_qp), ("vjp_qp", vjp_qp))
    times = {name: [] for name, _ in calls}
    for k in range(a.warmup + a.reps):
        for name, fn in calls:
            pt["clone"] = tuple(t.clone() for t in (x, y, s))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            if k >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    res = dict(config="C2 native (box QP)", B=B, n=tpl.n, m=tpl.m, nnz_p=eng.nnz_p, eps=a.eps, reps=a.reps, warmup=a.warmup,
               qp_ns_variant=int(_lib.lib().ce_qp_ns_variant(eng._h)), brt_variant=eng.plan()["brt_variant"])
    for name, _ in calls:
        t = np.asarray(times[name])
        res[name] = dict(ms_mean=float(t.mean()), ms_median=float(np.median(t)), ms_min=float(t.min()), ms_max=float(t.max()))
    res["jvp_qp"]["flagged_share"] = float(((last["jvp_qp"].cpu().numpy() & 4) != 0).mean())
    rst = last["refine_qp"].cpu().numpy()
    res["refine_qp_one_step"].update(kept_share=float(((rst & 1) != 0).mean()), rejected_share=float(((rst & 2) != 0).mean()), flagged_share=float(((rst & 4) != 0).mean()))
    res["vjp_qp"]["flagged_share"] = float((last["vjp_qp"].cpu().numpy() != 0).mean())
    res["time_ratio_jvp_qp_over_vjp_qp"] = res["jvp_qp"]["ms_mean"] / res["vjp_qp"]["ms_mean"]
    res["time_ratio_refine_step_over_vjp_qp"] = res["refine_qp_one_step"]["ms_mean"] / res["vjp_qp"]["ms_mean"]
    res["note"] = ("each call includes its host-side allocations; vjp_qp writes the batch-major dA and dP outputs, jvp_qp reads the tangent rows of the same sizes; "
                   "events on the launch stream; the LP pair ce_jvp / ce_vjp at the metric shape is 1.17 (DESIGN.md 3.3)")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
