"""Time of the one-instance-per-wave forward derivative and Newton refinement step (ce_jvp_wave, ce_refine_wave: k_newton_wave) against the ordinary routes
(ce_jvp, ce_refine) on small templates, one job, one box (profiles/newton_wave/newton_wave.json).

  families: scripts/fwd_wave_timing.py's seeded shapes (n, m) = (2, 3), (4, 8), (8, 16), (16, 32), (32, 64); points from the eps 1e-8 forward of the base batch,
            tiled to B = 4096 and 65536; Gaussian tangents of the value rows and of q_eval.
  routes: "wave" = ce_jvp_wave / ce_refine_wave, "workgroup" = ce_jvp / ce_refine of this build, "parent" = the same entries of the parent commit's library
          (--parent-so: loaded beside this one's); alternating inside every repetition, HIP events around the call (the LSQR re-solve launch is part of every
          forward-derivative route), medians of --reps with min - max.  A refinement call is ONE step on a fresh copy of the point (the copy is outside the events).
  per case: the share of flagged instances per route, the largest difference of dx between wave and workgroup on the unflagged instances, the share of kept steps,
            the resident workgroups per CU of both instantiations (ce_newton_wave_occupancy).
  layer: forward + backward of a scalar loss (parameters A, b, c) at (16, 32), B = 65536, eps 1e-4 and refine_steps 2: forward_kernel + adjoint_kernel alone
         against all three wave keys; wall ms around the synchronised step.

    python scripts/newton_wave_timing.py [--reps 30] [--warmup 3] [--parent-so PATH] [--out profiles/newton_wave/newton_wave.json] [--skip-layer] [--budget-s S]
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
from fwd_wave_timing import BASE_B, BATCHES, SEED, SHAPES, Parent, stats  # noqa: E402

TWO = {"forward_kernel": "wave", "adjoint_kernel": "wave"}
LAYER_KEYS = {"forward+adjoint": TWO, "all_three": {**TWO, "newton_kernel": "wave"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-so", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newton_wave", "newton_wave.json"))
    ap.add_argument("--skip-layer", action="store_true")
    ap.add_argument("--budget-s", type=float, default=0.0, help="> 0: a case that would start after this many seconds is not measured (listed under not_measured)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    parent = Parent(a.parent_so) if a.parent_so else None
    if parent:
        parent.L.ce_jvp.argtypes = L.ce_jvp.argtypes
        parent.L.ce_refine.argtypes = L.ce_refine.argtypes
    props = torch.cuda.get_device_properties(0)
    res = dict(device=props.name, cus=props.multi_processor_count, reps=a.reps, warmup=a.warmup, parent=bool(parent), base_batch=BASE_B, seed=SEED, cases=[], layer=None, not_measured=[])
    t_start = time.time()
    over = lambda: a.budget_s > 0 and time.time() - t_start > a.budget_s

    def dump():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    f64 = dict(dtype=torch.float64, device=dev)
    ctxs = []
    for n, cones in SHAPES:
        tpl = P.dense_template(n, cones)
        A, b, c = P.generate(n, cones, BASE_B, seed=SEED)
        A_eval, q_eval = tpl.values_from_dense(A, b, c)
        eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, cones, dev)
        A0, q0 = torch.from_numpy(np.ascontiguousarray(A_eval.T)).to(dev), torch.from_numpy(q_eval).to(dev)
        x, y, s, _, status, _ = eng.solve(A0, q0, make_settings(dict(eps=1e-8, max_iters=20000)))
        rng = np.random.default_rng(SEED + 1)
        ctxs.append(dict(tpl=tpl, cones=cones, eng=eng, hp=parent.create(tpl) if parent else None, occ=[int(L.ce_newton_wave_occupancy(eng._h, r)) for r in (0, 1)], A0=A0, q0=q0,
                         pt=(x, y, s), solved=int((status == 1).sum()),
                         tan=(torch.from_numpy(rng.standard_normal((BASE_B, tpl.nnz_aug))).to(dev), torch.from_numpy(rng.standard_normal((n + 1, BASE_B))).to(dev))))

    def timed(routes, before=None):
        ms = {r: [] for r, _ in routes}
        for rep in range(a.warmup + a.reps):
            for r, fn in routes:
                if before:
                    before(r)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record(); fn(); e1.record()
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    ms[r].append(e0.elapsed_time(e1))
        return ms

    def sweep(B):
        for cx in ctxs:
            tpl, cones, eng, hp = cx["tpl"], cx["cones"], cx["eng"], cx["hp"]
            if over():
                res["not_measured"].append(dict(n=tpl.n, m=tpl.m, B=B)); dump()
                continue
            variant, lds = eng.newton_wave_plan()
            k = B // BASE_B
            A_bm = cx["A0"].repeat(k, 1).contiguous(); q_t = cx["q0"].repeat(1, k).contiguous()
            x, y, s, tA = (t.repeat(k, 1).contiguous() for t in (*cx["pt"], cx["tan"][0]))
            tq = cx["tan"][1].repeat(1, k).contiguous()
            names = ("wave", "workgroup") + (("parent",) if parent else ())
            fns = dict(wave=(L.ce_jvp_wave, L.ce_refine_wave, eng._h), workgroup=(L.ce_jvp, L.ce_refine, eng._h))
            if parent:
                fns["parent"] = (parent.L.ce_jvp, parent.L.ce_refine, hp)
            q_args = (q_t.data_ptr(), q_t.stride(0), q_t.stride(1))
            # ---- the forward derivative
            out = {r: dict(dx=torch.empty((B, tpl.n), **f64), dy=torch.empty((B, tpl.m), **f64), ds=torch.empty((B, tpl.m), **f64),
                           st=torch.empty((B,), dtype=torch.int32, device=dev), it=torch.empty((B,), dtype=torch.int32, device=dev)) for r in names}

            def jvp(r):
                o = out[r]
                rc = fns[r][0](fns[r][2], B, A_bm.data_ptr(), tpl.nnz_aug, *q_args, x.data_ptr(), y.data_ptr(), s.data_ptr(), tA.data_ptr(), tpl.nnz_aug, tq.data_ptr(), tq.stride(0), tq.stride(1),
                               o["dx"].data_ptr(), o["dy"].data_ptr(), o["ds"].data_ptr(), o["st"].data_ptr(), o["it"].data_ptr(), 1e-8, 1e-8, 1e8, 0, stream)
                assert rc == 0, L.ce_last_error()
            ms_j = timed([(r, (lambda r=r: jvp(r))) for r in names])
            clean = (out["wave"]["st"] == 0) & (out["workgroup"]["st"] == 0)
            diff = float(((out["wave"]["dx"] - out["workgroup"]["dx"]).abs().amax(dim=1) / (1 + out["workgroup"]["dx"].abs().amax(dim=1)))[clean].max()) if bool(clean.any()) else None
            # ---- one refinement step from the solver's point
            pts = {r: None for r in names}
            rec = {r: dict(rst=torch.empty((B,), dtype=torch.int32, device=dev), taken=torch.empty((B,), dtype=torch.int32, device=dev), resid=torch.empty((B, 2), **f64)) for r in names}

            def fresh(r):
                pts[r] = (x.clone(), y.clone(), s.clone())

            def refine(r):
                o = rec[r]
                rc = fns[r][1](fns[r][2], B, A_bm.data_ptr(), tpl.nnz_aug, *q_args, *(t.data_ptr() for t in pts[r]), None, 1, o["rst"].data_ptr(), o["taken"].data_ptr(), o["resid"].data_ptr(), stream)
                assert rc == 0, L.ce_last_error()
            ms_r = timed([(r, (lambda r=r: refine(r))) for r in names], before=fresh)
            case = dict(n=tpl.n, m=tpl.m, cones=cones, B=B, variant=variant, lds_bytes=lds, resident_workgroups_per_cu=dict(jvp=cx["occ"][0], refine=cx["occ"][1]),
                        solved_share_of_base=cx["solved"] / BASE_B,
                        jvp_ms={r: stats(v) for r, v in ms_j.items()}, refine_ms={r: stats(v) for r, v in ms_r.items()},
                        jvp_flagged_share={r: float((out[r]["st"] != 0).double().mean()) for r in names}, max_rel_dx_difference_wave_workgroup_unflagged=diff,
                        refine_kept_share={r: float(((rec[r]["rst"] & 1) != 0).double().mean()) for r in names},
                        refine_rho_after_max={r: float(rec[r]["resid"][:, 1].max()) for r in names})
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            dump()

    sweep(BATCHES[0])
    if not a.skip_layer and over():
        res["not_measured"].append("layer"); dump()
    elif not a.skip_layer:
        from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
        from cvxpylayers_amd.torch.templates import template_from_affine_builder
        n, cones = SHAPES[3]; m = P.cone_rows(cones); B = 65536
        layer = CvxpyLayer(template=template_from_affine_builder(lambda A, b, c: (A, b, c), [(m, n), (m,), (n,)], cones, [VariableRecovery(slice(0, n), None, (n,))]),
                           solver_args={"eps": 1e-4, "max_iters": 20000, "refine_steps": 2})
        A, b, c = P.generate(n, cones, BASE_B, seed=SEED)
        ps = [torch.from_numpy(np.ascontiguousarray(np.tile(v, (B // BASE_B,) + (1,) * (v.ndim - 1)))).to(dev).requires_grad_(True) for v in (A, b, c)]
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
            for key in ms:
                t = step(key)
                if rep >= a.warmup:
                    ms[key].append(t)
                assert layer.info["refine"].get("kernel") == ("k_newton_wave" if "newton_kernel" in LAYER_KEYS[key] else None)
        res["layer"] = dict(n=n, m=m, cones=cones, B=B, eps=1e-4, refine_steps=2, what="forward + two refinement steps + backward of sum(x^2), parameters (A, b, c), wall ms",
                            ms={k: stats(v) for k, v in ms.items()})
        print(json.dumps(res["layer"]), flush=True)
        dump()
    for B in BATCHES[1:]:
        sweep(B)


if __name__ == "__main__":
    main()
