"""Time of the search-free elimination with PSD blocks at the LQR-like shape (n = 24, zero 3, nonnegative 2, PSD(6) + PSD(4)): the forward derivative by direct
elimination (ce_jvp_psd: k_backward_ns<..., FWD, ..., PSD> + the LSQR re-solve launch) next to the LSQR forward derivative (ce_jvp_lsqr), one Newton refinement
step (ce_refine_psd) and the pivoting adjoint (ce_vjp: k_backward_rt<PSD>, which keeps serving these templates in reverse mode) -- same point, diffcp's stopping
rule (1e-8 / 1e-8 / 1e8 / 2 N), same process, on the protocol of scripts/jvp_tri_timing.py: events on the launch stream around each call, warm-up calls first, then
--reps timed calls each, interleaved so that clock drift hits all; median, min, max in ms.  Then what refinement buys: the solve at eps = 1e-4 plus two refinement
steps against the solve at eps = 1e-8, each with its time and the largest distance of x to the oracle's eps = 1e-10 point on a 64-instance sample.
Prints one JSON line; --out also writes it to a file.

    python scripts/jvp_psd_timing.py [--B 4096] [--reps 30] [--warmup 5] [--out profiles/jvp/jvp_psd_direct.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cvxpylayers_amd import problems as P  # noqa: E402
from cvxpylayers_amd.interfaces.mi355_if import ConeEngine, make_settings  # noqa: E402


def _stats(t):
    t = np.asarray(t)
    return dict(ms_median=float(np.median(t)), ms_min=float(t.min()), ms_max=float(t.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sample", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from oracle import oracle
    n, cones, B = 24, {"z": 3, "l": 2, "q": [], "s": [6, 4]}, a.B          # (tests/psd_ns_kit.py lqr_like)
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=11)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, cones, torch.device("cuda", 0))
    A_bm = torch.from_numpy(A_eval).cuda().t().contiguous(); q_t = torch.from_numpy(q_eval).cuda()
    settings = {eps: make_settings(dict(eps=eps, max_iters=200000)) for eps in (1e-4, 1e-8)}
    x, y, s, _, status, _ = eng.solve(A_bm, q_t, settings[1e-8])
    solved = status == 1
    rng = np.random.default_rng(1)
    xb = torch.from_numpy(rng.standard_normal((B, tpl.n))).cuda(); yb = torch.zeros((B, tpl.m), dtype=torch.float64, device="cuda")
    tA = torch.from_numpy(rng.standard_normal((B, tpl.nnz_aug))).cuda(); tq = torch.from_numpy(rng.standard_normal((tpl.n + 1, B))).cuda()
    last = {}

    def direct():
        last["direct"] = (eng.jvp(A_bm, x, y, s, tA, tq, path="per_instance", q_eval=q_t, method="direct", psd_ns=True)[3], eng.last_lsqr_iters)
        assert eng.last_jvp_kernel == "ce_jvp_psd"

    def lsqr():
        last["lsqr"] = (eng.jvp(A_bm, x, y, s, tA, tq, path="per_instance", q_eval=q_t)[3], eng.last_lsqr_iters)

    def refine():
        last["refine"] = eng.refine(A_bm, q_t, x.clone(), y.clone(), s.clone(), 1, status=status, psd_ns=True)[3]
        assert last["refine"]["path"] == "ns"

    def vjp():
        last["vjp"] = (eng.vjp(A_bm, x, y, s, xb, yb, path="per_instance", q_eval=q_t)[2], None)

    def solve_refined():
        x4, y4, s4, _, st4, _ = eng.solve(A_bm, q_t, settings[1e-4])
        last["solve_1e-4_plus_two_steps"] = eng.refine(A_bm, q_t, x4, y4, s4, 2, status=st4, psd_ns=True)[:3] + (st4,)

    def solve_tight():
        x8, y8, s8, _, st8, _ = eng.solve(A_bm, q_t, settings[1e-8])
        last["solve_1e-8"] = (x8, y8, s8, st8)
    calls = (("jvp_direct", direct), ("jvp_lsqr", lsqr), ("refine_one_step", refine), ("vjp_pivoting", vjp), ("solve_1e-4_plus_two_steps", solve_refined), ("solve_1e-8", solve_tight))
    times = {name: [] for name, _ in calls}
    for k in range(a.warmup + a.reps):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            if k >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    plan = eng.psd_ns_plan()
    res = dict(config="lqr_like", cones=cones, B=B, n=tpl.n, m=tpl.m, rule="1e-8/1e-8/1e8/2N", reps=a.reps, warmup=a.warmup, psd_ns_variant=plan["psd_ns_variant"], psd_ns_lds=plan["psd_ns_lds"],
               point="engine solve at eps 1e-8", solved_share=float(solved.double().mean()))
    for name, _ in calls:
        res[name] = _stats(times[name])
    st, its = (t.cpu().numpy() for t in last["direct"])
    fl = (st & 8) != 0
    res["jvp_direct"].update(flagged_share=float(fl.mean()), flagged=int(fl.sum()), mean_lsqr_iters_of_flagged=float(its[fl].mean()) if fl.any() else 0.0,
                             not_converged=int(((st & 3) != 0).sum()))
    res["jvp_lsqr"]["mean_lsqr_iters"] = float(last["lsqr"][1].double().mean())
    rst = last["refine"]["status"].cpu().numpy()
    res["refine_one_step"].update(kept_share=float(((rst & 1) != 0).mean()), flagged_share=float(((rst & 4) != 0).mean()), rejected_share=float(((rst & 2) != 0).mean()))
    res["vjp_pivoting"]["flagged_share"] = float(((last["vjp"][0].cpu().numpy() & 8) != 0).mean())
    res["time_ratio_lsqr_over_direct"] = res["jvp_lsqr"]["ms_median"] / res["jvp_direct"]["ms_median"]
    res["time_ratio_direct_over_vjp"] = res["jvp_direct"]["ms_median"] / res["vjp_pivoting"]["ms_median"]
    # distance of x to the oracle's eps = 1e-10 point on a sample
    k = min(a.sample, B)
    hi = oracle.solve_batch(A[:k], b[:k], c[:k], cones, eps=1e-10, max_iters=200000)
    ok = hi["status"] == 1
    for name in ("solve_1e-4_plus_two_steps", "solve_1e-8"):
        xs, st_ = last[name][0][:k].cpu().numpy(), last[name][3][:k].cpu().numpy()
        use = ok & (st_ >= 0)
        res[name].update(sample=int(use.sum()), max_x_distance_to_oracle=float(np.abs(xs - hi["x"])[use].max()), median_x_distance_to_oracle=float(np.median(np.abs(xs - hi["x"]).max(axis=1)[use])))
    res["time_ratio_tight_solve_over_refined_solve"] = res["solve_1e-8"]["ms_median"] / res["solve_1e-4_plus_two_steps"]["ms_median"]
    res["note"] = ("each call includes its host-side allocations; vjp writes the batch-major dA output (B x nnz_aug doubles), the forward derivatives read the "
                   "tangent rows of the same size; refine_one_step includes three device copies of the point; events on the launch stream")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
