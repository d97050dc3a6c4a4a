"""Time of the forward derivative by direct elimination (ce_jvp: k_backward_ns<..., FWD> + the LSQR re-solve launch) next to the LSQR forward derivative
(ce_jvp_lsqr) and the default adjoint (ce_vjp, the yardstick: the same elimination in reverse mode) at the metric configuration: same shape, same point, diffcp's
stopping rule (1e-8 / 1e-8 / 1e8 / 2 N), same process.  Events on the launch stream around each call; warm-up calls first, then --reps timed calls each, the three
interleaved so that clock drift hits all.  Prints one JSON line (median, min, max in ms; the share of instances the elimination flagged and the mean LSQR
iterations of their re-solve; ratios); --out also writes it to a file.

    python scripts/jvp_direct_timing.py [--B 4096] [--reps 20] [--warmup 5] [--eps 1e-8] [--out profiles/jvp/jvp_direct_vs_lsqr_M.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=P.CONFIGS["M"]["B"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eps", type=float, default=1e-8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = P.CONFIGS["M"]; n, cones, B = cfg["n"], cfg["cones"], a.B
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=11)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, cones, torch.device("cuda", 0))
    A_bm = torch.from_numpy(A_eval).cuda().t().contiguous(); q_t = torch.from_numpy(q_eval).cuda()
    x, y, s, _, status, _ = eng.solve(A_bm, q_t, make_settings(dict(eps=a.eps, acceleration_lookback=0, max_iters=100000)))
    assert (status == 1).all()
    rng = np.random.default_rng(1)
    xb = torch.from_numpy(rng.standard_normal((B, tpl.n))).cuda(); yb = torch.zeros((B, tpl.m), dtype=torch.float64, device="cuda")
    tA = torch.from_numpy(rng.standard_normal((B, tpl.nnz_aug))).cuda(); tq = torch.from_numpy(rng.standard_normal((tpl.n + 1, B))).cuda()
    last = {}

    def direct():
        last["direct"] = (eng.jvp(A_bm, x, y, s, tA, tq, path="per_instance", q_eval=q_t, method="direct")[3], eng.last_lsqr_iters)
        assert eng.last_jvp_kernel == "ce_jvp"

    def lsqr():
        last["lsqr"] = (eng.jvp(A_bm, x, y, s, tA, tq, path="per_instance", q_eval=q_t)[3], eng.last_lsqr_iters)

    def vjp():
        last["vjp"] = (eng.vjp(A_bm, x, y, s, xb, yb, path="per_instance", q_eval=q_t)[2], None)
    calls = (("jvp_direct", direct), ("jvp_lsqr", lsqr), ("vjp_default", vjp))
    times = {name: [] for name, _ in calls}
    for k in range(a.warmup + a.reps):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            if k >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    res = dict(config="M", B=B, n=tpl.n, m=tpl.m, eps=a.eps, rule="1e-8/1e-8/1e8/2N", reps=a.reps, warmup=a.warmup, ns_variant=eng.plan()["ns_variant"])
    for name, _ in calls:
        t = np.asarray(times[name])
        res[name] = dict(ms_median=float(np.median(t)), ms_min=float(t.min()), ms_max=float(t.max()))
    st, its = (t.cpu().numpy() for t in last["direct"])
    fl = (st & 8) != 0
    res["jvp_direct"].update(flagged_share=float(fl.mean()), flagged=int(fl.sum()), mean_lsqr_iters_of_flagged=float(its[fl].mean()) if fl.any() else 0.0,
                             not_converged=int(((st & 3) != 0).sum()))
    res["jvp_lsqr"]["mean_lsqr_iters"] = float(last["lsqr"][1].double().mean())
    res["vjp_default"]["flagged_share"] = float(((last["vjp"][0].cpu().numpy() & 8) != 0).mean())
    res["time_ratio_lsqr_over_direct"] = res["jvp_lsqr"]["ms_median"] / res["jvp_direct"]["ms_median"]
    res["time_ratio_direct_over_vjp"] = res["jvp_direct"]["ms_median"] / res["vjp_default"]["ms_median"]
    res["note"] = ("each call includes its host-side allocations; vjp writes the batch-major dA output (B x nnz_aug doubles), the forward derivatives read the "
                   "tangent rows of the same size; events on the launch stream")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
