"""Time of the one-instance-per-wave forward derivative and Newton refinement step of small quadratic programs (ce_jvp_qp_wave, ce_refine_qp_wave:
k_newton_wave_qp) against the workgroup kernels of the same build (ce_jvp_qp, ce_refine_qp: k_backward_ns<..., FWD[, REF], QP>, whose device code is the parent
commit's byte for byte), one process, one box (profiles/newton_wave_qp/newton_wave_qp.json).

  families: scripts/fwd_wave_qp_timing.py's seeded shapes (n, m) = (2, 3), (8, 16), (16, 32), (32, 64) with P_i = G_i G_i^T / n + 1/2 I (dense, positive definite,
            upper-triangle structure); points from the eps 1e-8 forward (ce_solve_qp) of the base batch for the forward derivative, from the eps 1e-4 forward for
            the refinement step, tiled to B = 65536; Gaussian tangents of the value rows, of q and of P.
  routes: "wave" and "workgroup" alternating inside every repetition, HIP events around the call, --warmup repetitions dropped; the order inside a repetition
          flips from one repetition to the next (even: wave first, odd: workgroup first) and the medians of the two orders are recorded beside the overall median
          with min - max, so that the run-to-run spread and any order effect are visible.  The refinement step works in place: every timed call starts from a
          fresh copy of the point, copied outside the events.
  per case: the share of flagged instances per route, the largest difference of dx between the routes on the unflagged instances (refinement: the share of
            instances that kept the step, the largest rho after), the resident workgroups per CU of the instantiation (ce_newton_wave_qp_occupancy).
  layer: forward + backward of a scalar loss through the box projection of scripts/fwd_wave_qp_timing.py (n = 16, 32 rows, B = 65536, eps 1e-4) with
         refine_steps = 2, with and without newton_kernel="wave", alone and beside the two other wave keys; wall ms around the synchronised step.

    python scripts/newton_wave_qp_timing.py [--reps 30] [--warmup 3] [--out profiles/newton_wave_qp/newton_wave_qp.json] [--skip-layer]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from cvxpylayers_amd import _lib  # noqa: E402
from cvxpylayers_amd import problems as P  # noqa: E402
from cvxpylayers_amd.interfaces.mi355_if import ConeEngine, make_settings  # noqa: E402
from fwd_wave_qp_timing import BASE_B, SEED, SHAPES, stats, upper_structure  # noqa: E402

BATCH = 65536
SIZES = (2, 8, 16, 32)          # n of the measured shapes of fwd_wave_qp_timing.SHAPES
WAVES = {"forward_kernel": "wave", "adjoint_kernel": "wave"}
LAYER_KEYS = {"refine": {"refine_steps": 2}, "refine+newton": {"refine_steps": 2, "newton_kernel": "wave"},
              "waves+refine": {"refine_steps": 2, **WAVES}, "waves+refine+newton": {"refine_steps": 2, "newton_kernel": "wave", **WAVES}}


def alternate(routes, reps, warmup, before=None):
    """ms per route and per order: the routes alternate inside a repetition, the order flips between repetitions; before(): untimed preparation of every call"""
    ms = {r: {"wave_first": [], "workgroup_first": []} for r, _ in routes}
    for rep in range(warmup + reps):
        order = routes if rep % 2 == 0 else routes[::-1]
        for r, fn in order:
            if before:
                before(r)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(); fn(); e1.record()
            torch.cuda.synchronize()
            if rep >= warmup:
                ms[r]["wave_first" if rep % 2 == 0 else "workgroup_first"].append(e0.elapsed_time(e1))
    return {r: dict(stats(v["wave_first"] + v["workgroup_first"]), median_wave_first=float(np.median(v["wave_first"])),
                    median_workgroup_first=float(np.median(v["workgroup_first"]))) for r, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newton_wave_qp", "newton_wave_qp.json"))
    ap.add_argument("--skip-layer", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    props = torch.cuda.get_device_properties(0)
    res = dict(device=props.name, cus=props.multi_processor_count, reps=a.reps, warmup=a.warmup, base_batch=BASE_B, batch=BATCH, seed=SEED, cases=[], layer=None)
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)

    def dump():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    k = BATCH // BASE_B
    for n, cones in SHAPES:
        if n not in SIZES:
            continue
        tpl = P.dense_template(n, cones)
        A, b, c = P.generate(n, cones, BASE_B, seed=SEED)
        G = np.random.default_rng(SEED + 1000).standard_normal((BASE_B, n, n))
        Pm = G @ G.transpose(0, 2, 1) / n + 0.5 * np.eye(n)
        p_idx, p_ptr = upper_structure(n)
        A_eval, q_eval = tpl.values_from_dense(A, b, c)
        eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, cones, dev, p_structure=(p_idx, p_ptr))
        variant, lds = eng.newton_wave_qp_plan()
        assert eng.qp_native and variant >= 0
        A0 = torch.from_numpy(np.ascontiguousarray(A_eval.T)).to(dev)
        q0 = torch.from_numpy(q_eval).to(dev)
        P0 = torch.from_numpy(np.ascontiguousarray(Pm[:, p_idx, np.repeat(np.arange(n), np.diff(p_ptr))])).to(dev)
        rng = np.random.default_rng(SEED + 1)
        tan = [torch.from_numpy(rng.standard_normal(s)).to(dev) for s in ((BASE_B, tpl.nnz_aug), (n + 1, BASE_B), (BASE_B, eng.nnz_p))]
        tight = eng.solve(A0, q0, make_settings(dict(eps=1e-8, max_iters=20000)), P_bm=P0)
        loose = eng.solve(A0, q0, make_settings(dict(eps=1e-4, max_iters=20000)), P_bm=P0)
        A_bm, P_bm, tA, tP = (t.repeat(k, 1).contiguous() for t in (A0, P0, tan[0], tan[2]))
        q_t, tq = q0.repeat(1, k).contiguous(), tan[1].repeat(1, k).contiguous()
        case = dict(n=tpl.n, m=tpl.m, cones=cones, B=BATCH, variant=variant, lds_bytes=lds,
                    resident_workgroups_per_cu=dict(forward_derivative=int(L.ce_newton_wave_qp_occupancy(eng._h, 0)), refinement=int(L.ce_newton_wave_qp_occupancy(eng._h, 1))),
                    solved_share_of_base=dict(eps1e_8=float((tight[4] == 1).double().mean()), eps1e_4=float((loose[4] == 1).double().mean())))

        # ---- the forward derivative at the eps 1e-8 points
        x, y, s = (t.repeat(k, 1).contiguous() for t in tight[:3])
        out = {r: dict(dx=torch.empty((BATCH, n), **f64), dy=torch.empty((BATCH, tpl.m), **f64), ds=torch.empty((BATCH, tpl.m), **f64), st=torch.empty((BATCH,), **i32),
                       it=torch.empty((BATCH,), **i32)) for r in ("wave", "workgroup")}

        def jvp(fn, o):
            rc = fn(eng._h, BATCH, A_bm.data_ptr(), tpl.nnz_aug, P_bm.data_ptr(), x.data_ptr(), y.data_ptr(), s.data_ptr(), tA.data_ptr(), tpl.nnz_aug,
                    tq.data_ptr(), BATCH, 1, tP.data_ptr(), o["dx"].data_ptr(), o["dy"].data_ptr(), o["ds"].data_ptr(), o["st"].data_ptr(), o["it"].data_ptr(), stream)
            assert rc == 0, L.ce_last_error()
        ms = alternate([("wave", lambda: jvp(L.ce_jvp_qp_wave, out["wave"])), ("workgroup", lambda: jvp(L.ce_jvp_qp, out["workgroup"]))], a.reps, a.warmup)
        clean = (out["wave"]["st"] == 0) & (out["workgroup"]["st"] == 0)
        dxw, dxg = out["wave"]["dx"], out["workgroup"]["dx"]
        case["forward_derivative"] = dict(ms=ms, speedup_of_medians=ms["workgroup"]["median"] / ms["wave"]["median"],
                                          flagged_share={r: float((out[r]["st"] != 0).double().mean()) for r in out},
                                          max_rel_dx_difference_unflagged=float(((dxw - dxg).abs().amax(dim=1) / (1 + dxg.abs().amax(dim=1)))[clean].max()) if bool(clean.any()) else None)

        # ---- one refinement step from the eps 1e-4 points (in place: a fresh copy per call, outside the events)
        start = [t.repeat(k, 1).contiguous() for t in loose[:3]]
        pt = {r: [t.clone() for t in start] for r in ("wave", "workgroup")}
        rec = {r: dict(rst=torch.empty((BATCH,), **i32), steps=torch.empty((BATCH,), **i32), resid=torch.empty((BATCH, 2), **f64)) for r in pt}

        def fresh(r):
            for t, t0 in zip(pt[r], start):
                t.copy_(t0)

        def refine(fn, r):
            rc = fn(eng._h, BATCH, A_bm.data_ptr(), tpl.nnz_aug, q_t.data_ptr(), BATCH, 1, P_bm.data_ptr(), *(t.data_ptr() for t in pt[r]), None, 1,
                    rec[r]["rst"].data_ptr(), rec[r]["steps"].data_ptr(), rec[r]["resid"].data_ptr(), stream)
            assert rc == 0, L.ce_last_error()
        ms = alternate([("wave", lambda: refine(L.ce_refine_qp_wave, "wave")), ("workgroup", lambda: refine(L.ce_refine_qp, "workgroup"))], a.reps, a.warmup, before=fresh)
        case["refinement_step"] = dict(ms=ms, speedup_of_medians=ms["workgroup"]["median"] / ms["wave"]["median"],
                                       kept_share={r: float(((rec[r]["rst"] & 1) == 1).double().mean()) for r in rec},
                                       flagged_share={r: float(((rec[r]["rst"] & 4) != 0).double().mean()) for r in rec},
                                       max_rho_before={r: float(rec[r]["resid"][:, 0].max()) for r in rec}, max_rho_after={r: float(rec[r]["resid"][:, 1].max()) for r in rec})
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        dump()

    if not a.skip_layer:
        from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
        from cvxpylayers_amd.torch.templates import template_from_affine_builder
        n, B = 16, 65536

        def builder(v, lo, hi):          # min 1/2 |x - v|^2, lo <= x <= hi
            return np.concatenate([-np.eye(n), np.eye(n)]), np.concatenate([-lo, hi]), -v, np.eye(n)
        layer = CvxpyLayer(template=template_from_affine_builder(builder, [(n,), (n,), (n,)], {"z": 0, "l": 2 * n, "q": [], "s": []}, [VariableRecovery(slice(0, n), None, (n,))]),
                           solver_args={"eps": 1e-4, "max_iters": 20000})
        rng = np.random.default_rng(SEED)
        ps = [torch.from_numpy(t).to(dev).requires_grad_(True) for t in (rng.standard_normal((B, n)), -0.5 - 0.5 * rng.random((B, n)), 0.5 + 0.5 * rng.random((B, n)))]
        ms = {key: [] for key in LAYER_KEYS}

        def step(key):
            for p in ps:
                p.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            (xo,) = layer(*ps, solver_args=LAYER_KEYS[key])
            (xo ** 2).sum().backward()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        for rep in range(a.warmup + a.reps):
            for key in (list(ms) if rep % 2 == 0 else list(ms)[::-1]):
                t = step(key)
                if rep >= a.warmup:
                    ms[key].append(t)
                assert layer.info["refine"].get("kernel") == ("k_newton_wave_qp" if "newton_kernel" in LAYER_KEYS[key] else None)
        res["layer"] = dict(n=n, m=2 * n, B=B, eps=1e-4, refine_steps=2, what="box projection: forward + two refinement steps + backward of sum(x^2), parameters (v, lo, hi), wall ms",
                            ms={key: stats(v) for key, v in ms.items()})
        print(json.dumps(res["layer"]), flush=True)
        dump()


if __name__ == "__main__":
    main()
