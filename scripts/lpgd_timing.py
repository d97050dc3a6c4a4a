"""Times of the LPGD backward (interfaces/lpgd.py; ce_lpgd_perturb, ce_lpgd_grad) next to what it replaces, in one process at the same points:
  kernels, at the metric configuration M (B = 4096) at the solution of --eps (run it at 1e-4 and at 1e-8):
    * ce_lpgd_grad in both dA layouts, next to one ce_value_vjp, to TWO ce_value_vjp calls plus a torch subtraction and scaling (the route it replaces: the
      condition is that it beats that route), and to ce_transpose of the same (B, nnz_aug) array;
    * ce_lpgd_perturb with and without dy;
  whole backward passes (ConeEngine level: what backward() of the plugin enqueues), same point:
    * lpgd_right and lpgd (tau = 0.1, rho = 0) next to the default ce_vjp, and to a COLD ce_solve of the same perturbed data: what the warm start buys;
  one PSD and one shared-A point (--points psd,shared_a: sdp_c4_batch at B = 1024, portfolio_c5_batch at one GPU's share 2048 of BASELINE's 16384; both share A
  over the batch and run the shared-A kernels): lpgd_right next to the LSQR adjoint those templates run.
HIP events on the launch stream around each call, warm-up calls first, interleaved rounds; medians with min and max.  Prints one JSON line; --out writes it.

    python scripts/lpgd_timing.py [--B 4096] [--reps 30] [--warmup 5] [--eps 1e-8] [--points psd,shared_a] [--out profiles/lpgd/lpgd_M.json]
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
from cvxpylayers_amd.interfaces.lpgd import lpgd_backward  # noqa: E402
from cvxpylayers_amd.interfaces.mi355_if import ConeEngine, make_settings  # noqa: E402

DEV = torch.device("cuda", 0)
F64 = dict(dtype=torch.float64, device=DEV)


def timed(calls, warmup, reps):
    times = {name: [] for name, _ in calls}
    for k in range(warmup + reps):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            if k >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return {name: dict(ms_median=float(np.median(t)), ms_min=float(np.min(t)), ms_max=float(np.max(t))) for name, t in times.items()}


def point_M(eps, B, warmup, reps):
    cfg = P.CONFIGS["M"]; n, cones = cfg["n"], cfg["cones"]
    tpl = P.dense_template(n, cones)
    m, K = tpl.m, tpl.nnz_aug
    A, b, c = P.generate(n, cones, B, seed=11)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    eng = ConeEngine(tpl.indices, tpl.indptr, n, m, cones, DEV)
    A_bm = torch.from_numpy(A_eval).to(DEV).t().contiguous(); q_t = torch.from_numpy(q_eval).to(DEV)
    st = make_settings(dict(eps=eps, max_iters=100000))
    x, y, s, it0, status, _ = eng.solve(A_bm, q_t, st)
    assert (status == 1).all()
    rng = np.random.default_rng(5)
    dx, dy = torch.from_numpy(rng.standard_normal((B, n))).to(DEV), torch.from_numpy(rng.standard_normal((B, m))).to(DEV)
    tau = 0.1
    # one perturbed point to difference against (the +tau side)
    q_p, A_p, _, _ = eng.lpgd_perturb(A_bm, q_t, x, dx, dy, tau, 0.0)
    xp, yp, sp, it_warm, st_w, _ = eng.solve_transient(A_p, q_p, st, warm=(x, y, s))
    xc, yc, sc, it_cold, st_c, _ = eng.solve_transient(A_p, q_p, st)
    L, h, sm = _lib.lib(), eng._h, eng._stream()
    g1 = torch.full((B,), 1.0 / tau, **F64)
    dA1, dA2, dA3, tr_out = (torch.empty(B * K, **F64) for _ in range(4))
    dq1, dq2, dq3 = (torch.empty((n + 1) * B, **F64) for _ in range(3))
    q_out, A_out = torch.empty_like(q_t), torch.empty_like(A_bm)
    flags = torch.empty(B, dtype=torch.int32, device=DEV)

    def grad(sk, sb, sqk, sqb):
        return lambda: _lib.check(L.ce_lpgd_grad(h, B, x.data_ptr(), y.data_ptr(), xp.data_ptr(), yp.data_ptr(), tau, None, dA1.data_ptr(), sk, sb,
                                                 dq1.data_ptr(), sqk, sqb, None, None, None, 0, sm), "ce_lpgd_grad")

    def vjp(g, dA, dq, px, py, sk, sb, sqk, sqb):
        _lib.check(L.ce_value_vjp(h, B, px.data_ptr(), py.data_ptr(), g.data_ptr(), None, dA.data_ptr(), sk, sb, dq.data_ptr(), sqk, sqb, None, None, None, 0, sm), "ce_value_vjp")

    def two_vjp(sk, sb, sqk, sqb):
        def run():
            vjp(g1, dA2, dq2, xp, yp, sk, sb, sqk, sqb); vjp(g1, dA3, dq3, x, y, sk, sb, sqk, sqb)
            return dA2 - dA3, dq2 - dq3
        return run

    def perturb(with_dy):
        return lambda: _lib.check(L.ce_lpgd_perturb(h, B, A_bm.data_ptr(), K, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), None, None, None, 0, x.data_ptr(), dx.data_ptr(),
                                                    dy.data_ptr() if with_dy else None, tau, 0.0, q_out.data_ptr(), A_out.data_ptr(), None, flags.data_ptr(), sm), "ce_lpgd_perturb")
    major, minor = (1, K, 1, n + 1), (B, 1, B, 1)
    calls = (("lpgd_grad_batch_major", grad(*major)), ("lpgd_grad_batch_minor", grad(*minor)),
             ("value_vjp_batch_major", lambda: vjp(g1, dA2, dq2, x, y, *major)), ("value_vjp_batch_minor", lambda: vjp(g1, dA2, dq2, x, y, *minor)),
             ("two_value_vjp_and_subtract_batch_major", two_vjp(*major)), ("two_value_vjp_and_subtract_batch_minor", two_vjp(*minor)),
             ("transpose", lambda: _lib.check(L.ce_transpose(h, B, K, dA1.data_ptr(), tr_out.data_ptr(), sm), "ce_transpose")),
             ("lpgd_perturb_with_dy", perturb(True)), ("lpgd_perturb_without_dy", perturb(False)),
             ("backward_lpgd_right", lambda: lpgd_backward(eng, ("lpgd_right", tau, 0.0), st, "per_instance", A_bm, q_t, None, x, y, s, dx, dy)),
             ("backward_lpgd_central", lambda: lpgd_backward(eng, ("lpgd", tau, 0.0), st, "per_instance", A_bm, q_t, None, x, y, s, dx, dy)),
             ("backward_default_ce_vjp", lambda: eng.vjp(A_bm, x, y, s, dx, dy, path="per_instance", q_eval=q_t)),
             ("perturbed_solve_warm", lambda: eng.solve_transient(A_p, q_p, st, warm=(x, y, s))), ("perturbed_solve_cold", lambda: eng.solve_transient(A_p, q_p, st)))
    res = timed(calls, warmup, reps)
    # the routes computed the same thing
    grad(*major)(); d_new = dA1.clone(); d_old = two_vjp(*major)()[0]
    rel = float((d_new - d_old).abs().max() / d_old.abs().max())
    bytes_grad = 8.0 * B * (K + (n + 1))
    for k in ("lpgd_grad_batch_major", "lpgd_grad_batch_minor"):
        res[k].update(bytes_written=bytes_grad, tb_per_s_of_bytes_written=bytes_grad / (res[k]["ms_median"] * 1e-3) / 1e12)
    res.update(config="M", B=B, n=n, m=m, nnz_aug=K, eps=eps, tau=tau, forward_iters_mean=float(it0.double().mean()), perturbed_iters_warm_mean=float(it_warm.double().mean()),
               perturbed_iters_cold_mean=float(it_cold.double().mean()), perturbed_solved=bool(((st_w > 0) & (st_c > 0)).all()), max_rel_diff_grad_vs_two_vjp=rel,
               condition_lpgd_grad_beats_two_vjp_and_subtract=bool(res["lpgd_grad_batch_major"]["ms_median"] < res["two_value_vjp_and_subtract_batch_major"]["ms_median"] and
                                                                   res["lpgd_grad_batch_minor"]["ms_median"] < res["two_value_vjp_and_subtract_batch_minor"]["ms_median"]))
    return res


def point_other(which, eps, warmup, reps):
    """lpgd_right next to the shared-A LSQR adjoint these templates run"""
    if which == "psd":
        B = P.CONFIGS["C4"]["B"]
        A1, b, c, cones, tpl = P.sdp_c4_batch(B)
    else:
        B = 2048
        A1, b1, c, cones, tpl = P.portfolio_c5_batch(B)
        b = np.broadcast_to(b1, (B, len(b1))).copy()
    # (A is shared: the values of one instance, repeated; only the b entries and q differ -- no dense (B, m, n) array is formed)
    A_eval = np.repeat(tpl.values_from_dense(A1[None], b[:1], c[:1])[0], B, axis=1)
    b_slots = np.arange(tpl.indptr[tpl.n], tpl.indptr[tpl.n + 1])
    A_eval[b_slots] = b[:, np.asarray(tpl.indices)[b_slots]].T
    q_eval = np.ascontiguousarray(np.concatenate([c.T, np.zeros((1, B))], axis=0))
    eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, cones, DEV, A_is_constant=True)          # (both batches share A: the dispatcher takes the shared-A path, as BASELINE's runs do)
    A_bm = torch.from_numpy(A_eval).to(DEV).t().contiguous(); q_t = torch.from_numpy(q_eval).to(DEV)
    st = make_settings(dict(eps=eps, max_iters=100000))
    x, y, s, it0, status, _ = eng.solve(A_bm, q_t, st)
    path = eng.last_path
    rng = np.random.default_rng(5)
    dx = torch.from_numpy(0.1 * rng.standard_normal((B, tpl.n))).to(DEV)          # (tau dx = 0.01 N(0, 1) on c: a larger step makes many perturbed SDPs unbounded -- bit 16, counted below)
    calls = (("backward_lpgd_right", lambda: lpgd_backward(eng, ("lpgd_right", 0.1, 0.0), st, path, A_bm, q_t, None, x, y, s, dx, None)),
             ("backward_default_adjoint", lambda: eng.vjp(A_bm, x, y, s, dx, eng.zeros_like_cached(y), path=path, q_eval=q_t)))
    res = timed(calls, min(warmup, 1), min(reps, 5))
    _, _, _, stt, its = lpgd_backward(eng, ("lpgd_right", 0.1, 0.0), st, path, A_bm, q_t, None, x, y, s, dx, None)
    res.update(B=B, n=tpl.n, m=tpl.m, eps=eps, path=path, forward_solved_share=float((status > 0).double().mean()), forward_iters_mean=float(it0.double().mean()),
               perturbed_iters_mean=float(its.double().mean()), lpgd_status_nonzero=int((stt != 0).sum()),
               lpgd_right_beats_the_lsqr_adjoint=bool(res["backward_lpgd_right"]["ms_median"] < res["backward_default_adjoint"]["ms_median"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=P.CONFIGS["M"]["B"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eps", type=float, nargs="+", default=[1e-4, 1e-8])
    ap.add_argument("--points", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lpgd_timing.py measures on the GPU; there is nothing to fall back to")
    res = {f"M_eps_{e:g}": point_M(e, a.B, a.warmup, a.reps) for e in a.eps}
    for which in [w for w in a.points.split(",") if w]:
        res[which] = point_other(which, 1e-4, a.warmup, a.reps)
    res["note"] = ("events on the launch stream around each call; kernel rows go through the C ABI into buffers allocated beforehand, backward_* and perturbed_solve_* rows "
                   "through ConeEngine (their output allocations included, as in the plugin's backward); two_value_vjp_and_subtract includes the two torch subtractions")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    bad = [k for k, v in res.items() if isinstance(v, dict) and v.get("condition_lpgd_grad_beats_two_vjp_and_subtract") is False]
    if bad:
        raise SystemExit(f"ce_lpgd_grad did not beat two ce_value_vjp calls plus a subtraction at {bad}")


if __name__ == "__main__":
    main()
