"""Time of the one-instance-per-wave adjoint of small quadratic programs (ce_vjp_qp_wave, k_bwd_wave_qp) against the ordinary route (ce_vjp_qp, the pivoting
kernel) on small templates, one job, one box (profiles/bwd_wave_qp/bwd_wave_qp.json).

  families: scripts/fwd_wave_qp_timing.py's seeded shapes (n, m) = (2, 3), (4, 8), (8, 16), (16, 32), (32, 64) with P_i = G_i G_i^T / n + 1/2 I (dense, positive
            definite, upper-triangle structure); points from the eps 1e-8 forward (ce_solve_qp) of the base batch, tiled to B = 4096 and 65536; Gaussian cotangents.
  routes: "wave" = ce_vjp_qp_wave, "workgroup" = ce_vjp_qp of this build, "parent" = ce_vjp_qp of the parent commit's library (--parent-so: loaded beside this
          one's); alternating inside every repetition, HIP events around the call, medians of --reps with min - max.
  per case: the share of flagged instances per route, the largest difference of dA and dP between wave and workgroup on the unflagged instances, the resident
            workgroups per CU of the instantiation (ce_bwd_wave_qp_occupancy).
  layer: forward + backward of a scalar loss through the box projection of scripts/fwd_wave_qp_timing.py (n = 16, 32 rows, B = 65536, eps 1e-4), three ways: no
         key, forward_kernel alone, both keys; wall ms around the synchronised step.

    python scripts/bwd_wave_qp_timing.py [--reps 30] [--warmup 3] [--parent-so PATH] [--out profiles/bwd_wave_qp/bwd_wave_qp.json] [--skip-layer] [--budget-s S]
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
from fwd_wave_qp_timing import BASE_B, BATCHES, SEED, SHAPES, Parent, stats, upper_structure  # noqa: E402

LAYER_KEYS = {"none": {}, "forward": {"forward_kernel": "wave"}, "both": {"forward_kernel": "wave", "adjoint_kernel": "wave"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-so", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bwd_wave_qp", "bwd_wave_qp.json"))
    ap.add_argument("--skip-layer", action="store_true")
    ap.add_argument("--budget-s", type=float, default=0.0, help="> 0: a case that would start after this many seconds is not measured (listed under not_measured)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    parent = Parent(a.parent_so) if a.parent_so else None
    if parent:
        parent.L.ce_vjp_qp.argtypes = L.ce_vjp_qp.argtypes
    props = torch.cuda.get_device_properties(0)
    res = dict(device=props.name, cus=props.multi_processor_count, reps=a.reps, warmup=a.warmup, parent=bool(parent), base_batch=BASE_B, seed=SEED, cases=[], layer=None, not_measured=[])
    t_start = time.time()
    over = lambda: a.budget_s > 0 and time.time() - t_start > a.budget_s

    def dump():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)

    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    ctxs = []
    for n, cones in SHAPES:
        tpl = P.dense_template(n, cones)
        A, b, c = P.generate(n, cones, BASE_B, seed=SEED)
        G = np.random.default_rng(SEED + 1000).standard_normal((BASE_B, n, n))
        Pm = G @ G.transpose(0, 2, 1) / n + 0.5 * np.eye(n)
        p_idx, p_ptr = upper_structure(n)
        A_eval, q_eval = tpl.values_from_dense(A, b, c)
        eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, cones, dev, p_structure=(p_idx, p_ptr))
        assert eng.qp_native and eng.bwd_wave_qp_plan()[0] >= 0
        A0 = torch.from_numpy(np.ascontiguousarray(A_eval.T)).to(dev)
        P0 = torch.from_numpy(np.ascontiguousarray(Pm[:, p_idx, np.repeat(np.arange(n), np.diff(p_ptr))])).to(dev)
        x, y, s, _, status, _ = eng.solve(A0, torch.from_numpy(q_eval).to(dev), make_settings(dict(eps=1e-8, max_iters=20000)), P_bm=P0)
        rng = np.random.default_rng(SEED + 1)
        ctxs.append(dict(tpl=tpl, cones=cones, eng=eng, hp=parent.create(tpl, p_idx, p_ptr) if parent else None, occ=int(L.ce_bwd_wave_qp_occupancy(eng._h)), A0=A0, P0=P0,
                         pt=(x, y, s), solved=int((status == 1).sum()), cot=(torch.from_numpy(rng.standard_normal((BASE_B, n))).to(dev), torch.from_numpy(rng.standard_normal((BASE_B, tpl.m))).to(dev))))

    def sweep(B):
        for cx in ctxs:
            tpl, cones, eng, hp = cx["tpl"], cx["cones"], cx["eng"], cx["hp"]
            if over():
                res["not_measured"].append(dict(n=tpl.n, m=tpl.m, B=B)); dump()
                continue
            variant, lds = eng.bwd_wave_qp_plan()
            k = B // BASE_B
            A_bm, P_bm, x, y, s, dx, dy = (t.repeat(k, 1).contiguous() for t in (cx["A0"], cx["P0"], *cx["pt"], *cx["cot"]))
            out = {r: dict(dA=torch.empty((B, tpl.nnz_aug), dtype=torch.float64, device=dev), dq=torch.empty((tpl.n + 1, B), dtype=torch.float64, device=dev),
                           dP=torch.empty((B, eng.nnz_p), dtype=torch.float64, device=dev), adj=torch.empty((B,), dtype=torch.int32, device=dev)) for r in ("wave", "workgroup", "parent")}

            def call(fn, h, o):
                rc = fn(h, B, A_bm.data_ptr(), 1, tpl.nnz_aug, P_bm.data_ptr(), x.data_ptr(), y.data_ptr(), s.data_ptr(), dx.data_ptr(), dy.data_ptr(),
                        o["dA"].data_ptr(), 1, tpl.nnz_aug, o["dq"].data_ptr(), B, 1, o["dP"].data_ptr(), o["adj"].data_ptr(), stream)
                assert rc == 0, L.ce_last_error()
            routes = [("wave", lambda: call(L.ce_vjp_qp_wave, eng._h, out["wave"])), ("workgroup", lambda: call(L.ce_vjp_qp, eng._h, out["workgroup"]))]
            if parent:
                routes.append(("parent", lambda: call(parent.L.ce_vjp_qp, hp, out["parent"])))
            ms = {r: [] for r, _ in routes}
            for rep in range(a.warmup + a.reps):
                for r, fn in routes:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record(); fn(); e1.record()
                    torch.cuda.synchronize()
                    if rep >= a.warmup:
                        ms[r].append(e0.elapsed_time(e1))
            clean = (out["wave"]["adj"] == 0) & (out["workgroup"]["adj"] == 0)
            rel = lambda f: float(((out["wave"][f] - out["workgroup"][f]).abs().amax(dim=1) / (1 + out["workgroup"][f].abs().amax(dim=1)))[clean].max()) if bool(clean.any()) else None
            case = dict(n=tpl.n, m=tpl.m, cones=cones, B=B, variant=variant, lds_bytes=lds, resident_workgroups_per_cu=cx["occ"], solved_share_of_base=cx["solved"] / BASE_B,
                        ms={r: stats(v) for r, v in ms.items()}, instances_per_s={r: B / (np.median(v) * 1e-3) for r, v in ms.items()},
                        flagged_share={r: float((out[r]["adj"] != 0).double().mean()) for r, _ in routes},
                        max_rel_dA_difference_wave_workgroup_unflagged=rel("dA"), max_rel_dP_difference_wave_workgroup_unflagged=rel("dP"))
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            dump()

    sweep(BATCHES[0])
    if not a.skip_layer and over():
        res["not_measured"].append("layer"); dump()
    elif not a.skip_layer:
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
            (xo,) = layer(*ps, solver_args=LAYER_KEYS[key] or None)
            (xo ** 2).sum().backward()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        for rep in range(a.warmup + a.reps):
            for key in ms:
                t = step(key)
                if rep >= a.warmup:
                    ms[key].append(t)
                assert layer.info["adjoint"].get("kernel") == ("k_bwd_wave_qp" if "adjoint_kernel" in LAYER_KEYS[key] else None)
        res["layer"] = dict(n=n, m=2 * n, B=B, eps=1e-4, what="box projection: forward + backward of sum(x^2), parameters (v, lo, hi), wall ms", ms={k: stats(v) for k, v in ms.items()})
        print(json.dumps(res["layer"]), flush=True)
        dump()
    for B in BATCHES[1:]:
        sweep(B)


if __name__ == "__main__":
    main()
