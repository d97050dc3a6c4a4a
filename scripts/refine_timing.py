"""Cost and effect of Newton refinement (ce_refine: k_backward_ns<..., FWD, REF>) at the metric configuration, one process, one box:
  * one refinement step next to the forward derivative by direct elimination (ce_jvp) and the default adjoint (ce_vjp) -- the same elimination in its three
    modes, at the same eps = 1e-4 point (every timed step starts from a fresh copy of that point, made outside the events);
  * the forward solve at eps = 1e-4 followed by 1 / 2 / 3 steps next to the forward solve at eps = 1e-8 and 1e-10;
  * for each of those, the error of x against the oracle at eps = 1e-11 on a sample of the batch (maximum and median over the sample of the per-instance
    max |x - x_ref| / (1 + max |x_ref|)) and the share of instances by refine_status.
Events on the launch stream around each call; warm-up calls first, then --reps timed calls each, interleaved.  Prints one JSON line; --out also writes it.

    python scripts/refine_timing.py [--B 4096] [--reps 20] [--warmup 5] [--sample 256] [--out profiles/refine/refine_M.json]
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
from oracle import oracle  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=P.CONFIGS["M"]["B"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sample", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cfg = P.CONFIGS["M"]; n, cones, B = cfg["n"], cfg["cones"], a.B
    tpl = P.dense_template(n, cones)
    A, b, c = P.generate(n, cones, B, seed=11)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, cones, torch.device("cuda", 0))
    A_bm = torch.from_numpy(A_eval).cuda().t().contiguous(); q_t = torch.from_numpy(q_eval).cuda()
    ns = min(a.sample, B)
    ref = oracle.solve_batch(A[:ns], b[:ns], c[:ns], cones, eps=1e-11, max_iters=200000)
    ref_ok = ref["status"] == 1

    def settings(eps):
        return make_settings(dict(eps=eps, max_iters=100000))

    def x_error(x):
        e = (np.abs(x[:ns].cpu().numpy() - ref["x"]).max(axis=1) / (1 + np.abs(ref["x"]).max(axis=1)))[ref_ok]
        return dict(x_err_max=float(e.max()), x_err_median=float(np.median(e)))

    def time_calls(calls, prepare=None):
        times = {name: [] for name, _ in calls}
        for k in range(a.warmup + a.reps):
            for name, fn in calls:
                if prepare is not None:
                    prepare()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record(); e1.synchronize()
                if k >= a.warmup:
                    times[name].append(e0.elapsed_time(e1))
        return {name: dict(ms_median=float(np.median(t)), ms_min=float(np.min(t)), ms_max=float(np.max(t))) for name, t in times.items()}

    res = dict(config="M", B=B, n=tpl.n, m=tpl.m, reps=a.reps, warmup=a.warmup, sample=int(ref_ok.sum()), ns_variant=eng.plan()["ns_variant"])
    # ---- the elimination in its three modes at the eps = 1e-4 point
    x0, y0, s0, _, status0, _ = eng.solve(A_bm, q_t, settings(1e-4))
    res["start_failed"] = int((status0 < 0).sum())          # (skipped by the refinement; none expected at this configuration)
    rng = np.random.default_rng(1)
    xb = torch.from_numpy(rng.standard_normal((B, tpl.n))).cuda(); yb = torch.zeros((B, tpl.m), dtype=torch.float64, device="cuda")
    tA = torch.from_numpy(rng.standard_normal((B, tpl.nnz_aug))).cuda(); tq = torch.from_numpy(rng.standard_normal((tpl.n + 1, B))).cuda()
    work = [t.clone() for t in (x0, y0, s0)]

    def fresh():
        for w, t in zip(work, (x0, y0, s0)):
            w.copy_(t)
    kernel = time_calls((("refine_one_step", lambda: eng.refine(A_bm, q_t, *work, 1, status=status0)),
                         ("jvp_direct", lambda: eng.jvp(A_bm, x0, y0, s0, tA, tq, path="per_instance", q_eval=q_t, method="direct")),
                         ("vjp_default", lambda: eng.vjp(A_bm, x0, y0, s0, xb, yb, path="per_instance", q_eval=q_t))), prepare=fresh)
    res.update(kernel)
    res["time_ratio_refine_over_jvp_direct"] = kernel["refine_one_step"]["ms_median"] / kernel["jvp_direct"]["ms_median"]
    # ---- forward + steps against tighter forward solves
    out = {}

    def fwd(eps, steps):
        def run():
            x, y, s, _, status, _ = eng.solve(A_bm, q_t, settings(eps))
            info = None
            if steps:
                x, y, s, info = eng.refine(A_bm, q_t, x, y, s, steps, status=status)
            out[(eps, steps)] = (x, info)
        return run
    plans = [("fwd_1e-4", 1e-4, 0), ("fwd_1e-4_refine_1", 1e-4, 1), ("fwd_1e-4_refine_2", 1e-4, 2), ("fwd_1e-4_refine_3", 1e-4, 3), ("fwd_1e-8", 1e-8, 0), ("fwd_1e-10", 1e-10, 0)]
    timed = time_calls([(name, fwd(eps, steps)) for name, eps, steps in plans])
    for name, eps, steps in plans:
        x, info = out[(eps, steps)]
        timed[name].update(x_error(x))
        if info is not None:
            st = info["status"].cpu().numpy(); r1 = info["resid_after"].cpu().numpy()
            timed[name].update(share_kept=float(((st & 1) != 0).mean()), share_rejected=float(((st & 2) != 0).mean()), share_flagged=float(((st & 4) != 0).mean()),
                               share_skipped=float(((st & 16) != 0).mean()), share_resid_le_1e_12=float((r1 <= 1e-12).mean()), resid_after_median=float(np.median(r1)),
                               steps_kept_mean=float(info["steps"].double().mean()))
    res.update(timed)
    res["note"] = ("each call includes its host-side allocations; events on the launch stream; the refinement step is timed from a fresh copy of the eps = 1e-4 point "
                   "(the copy is outside the events); default solver settings (Anderson acceleration on) for every forward solve")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
