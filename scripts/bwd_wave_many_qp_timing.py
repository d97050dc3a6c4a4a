"""Time of the many-cotangent wave adjoint of small quadratic programs (ce_vjp_qp_many_wave, k_bwd_wave_many_qp) against the routes it replaces, one job, one box
(profiles/bwd_wave_many_qp/bwd_wave_many_qp.json).

  families: scripts/fwd_wave_qp_timing.py's seeded shapes (n, m) = (2, 3), (8, 16), (16, 32), (32, 64) with P_i = G_i G_i^T / n + 1/2 I (dense, positive definite,
            upper-triangle structure); points from the eps 1e-8 forward (ce_solve_qp) of the base batch, tiled to B = 4096 and 65536; K = n Gaussian cotangents.
  routes: "wave_many" = ce_vjp_qp_many_wave, "workgroup_many" = ce_vjp_qp_many of this build, "parent_many" = ce_vjp_qp_many of the parent commit's library
          (--parent-so: loaded beside this one's), "wave_loop" = K calls of ce_vjp_qp_wave.  The routes alternate inside every repetition and the order flips
          between repetitions; HIP events around the call(s), medians of --reps with min - max.  The routes share one set of output buffers (K B nnz_aug doubles
          at n = 32, B = 65536 is 35 GB); every route's flags are read behind its last call.
  per case: the share of flagged pairs per route, the resident workgroups per CU of the instantiation (ce_bwd_wave_many_qp_occupancy), its LDS and chunk.
  layer: layer.jacobian(direction="reverse") of the box projection of scripts/bwd_wave_qp_timing.py (n = 16, 32 rows, B = 4096, eps 1e-8) under
         qp_adjoint="search_free" with and without adjoint_kernel="wave"; wall ms around the synchronised call.

    python scripts/bwd_wave_many_qp_timing.py [--reps 30] [--warmup 3] [--parent-so PATH] [--out profiles/bwd_wave_many_qp/bwd_wave_many_qp.json] [--skip-layer] [--n N ...] [--budget-s S]
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

LAYER_KEYS = {"search_free": {"qp_adjoint": "search_free"}, "search_free_wave": {"qp_adjoint": "search_free", "adjoint_kernel": "wave"}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-so", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bwd_wave_many_qp", "bwd_wave_many_qp.json"))
    ap.add_argument("--skip-layer", action="store_true")
    ap.add_argument("--n", type=int, nargs="*", default=None, help="measure these n alone (default: every shape)")
    ap.add_argument("--budget-s", type=float, default=0.0, help="> 0: a case that would start after this many seconds is not measured (listed under not_measured)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    parent = Parent(a.parent_so) if a.parent_so else None
    if parent:
        parent.L.ce_vjp_qp_many.argtypes = L.ce_vjp_qp_many.argtypes
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
        if n == 4 or (a.n and n not in a.n):
            continue
        tpl = P.dense_template(n, cones)
        A, b, c = P.generate(n, cones, BASE_B, seed=SEED)
        G = np.random.default_rng(SEED + 1000).standard_normal((BASE_B, n, n))
        Pm = G @ G.transpose(0, 2, 1) / n + 0.5 * np.eye(n)
        p_idx, p_ptr = upper_structure(n)
        A_eval, q_eval = tpl.values_from_dense(A, b, c)
        eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, cones, dev, p_structure=(p_idx, p_ptr))
        assert eng.qp_native and eng.bwd_wave_many_qp_plan()[0] >= 0
        A0 = torch.from_numpy(np.ascontiguousarray(A_eval.T)).to(dev)
        P0 = torch.from_numpy(np.ascontiguousarray(Pm[:, p_idx, np.repeat(np.arange(n), np.diff(p_ptr))])).to(dev)
        x, y, s, _, status, _ = eng.solve(A0, torch.from_numpy(q_eval).to(dev), make_settings(dict(eps=1e-8, max_iters=20000)), P_bm=P0)
        rng = np.random.default_rng(SEED + 1)
        ctxs.append(dict(tpl=tpl, cones=cones, eng=eng, hp=parent.create(tpl, p_idx, p_ptr) if parent else None, occ=int(L.ce_bwd_wave_many_qp_occupancy(eng._h)), A0=A0, P0=P0,
                         pt=(x, y, s), solved=int((status == 1).sum()),
                         cot=(torch.from_numpy(rng.standard_normal((n, BASE_B, n))).to(dev), torch.from_numpy(rng.standard_normal((n, BASE_B, tpl.m))).to(dev))))

    def sweep(B):
        for cx in ctxs:
            tpl, cones, eng, hp = cx["tpl"], cx["cones"], cx["eng"], cx["hp"]
            if over():
                res["not_measured"].append(dict(n=tpl.n, m=tpl.m, B=B)); dump()
                continue
            variant, lds, chunk = eng.bwd_wave_many_qp_plan()
            K, k = tpl.n, B // BASE_B
            A_bm, P_bm, x, y, s = (t.repeat(k, 1).contiguous() for t in (cx["A0"], cx["P0"], *cx["pt"]))
            dx, dy = (t.repeat(1, k, 1).contiguous() for t in cx["cot"])
            f64 = dict(dtype=torch.float64, device=dev)
            dA, dq, dP = torch.empty((K, B, tpl.nnz_aug), **f64), torch.empty((K, B, tpl.n + 1), **f64), torch.empty((K, B, eng.nnz_p), **f64)
            dq1, adj = torch.empty((tpl.n + 1, B), **f64), torch.empty((K, B), dtype=torch.int32, device=dev)

            def many(fn, h):
                rc = fn(h, B, K, A_bm.data_ptr(), tpl.nnz_aug, P_bm.data_ptr(), x.data_ptr(), y.data_ptr(), s.data_ptr(), dx.data_ptr(), dy.data_ptr(),
                        dA.data_ptr(), dq.data_ptr(), dP.data_ptr(), adj.data_ptr(), stream)
                assert rc == 0, L.ce_last_error()

            def loop():
                for i in range(K):
                    rc = L.ce_vjp_qp_wave(eng._h, B, A_bm.data_ptr(), 1, tpl.nnz_aug, P_bm.data_ptr(), x.data_ptr(), y.data_ptr(), s.data_ptr(), dx[i].data_ptr(), dy[i].data_ptr(),
                                          dA[i].data_ptr(), 1, tpl.nnz_aug, dq1.data_ptr(), B, 1, dP[i].data_ptr(), adj[i].data_ptr(), stream)
                    assert rc == 0, L.ce_last_error()
            routes = [("wave_many", lambda: many(L.ce_vjp_qp_many_wave, eng._h)), ("workgroup_many", lambda: many(L.ce_vjp_qp_many, eng._h)), ("wave_loop", loop)]
            if parent:
                routes.append(("parent_many", lambda: many(parent.L.ce_vjp_qp_many, hp)))
            ms, flagged = {r: [] for r, _ in routes}, {}
            for rep in range(a.warmup + a.reps):
                for r, fn in (routes if rep % 2 == 0 else routes[::-1]):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record(); fn(); e1.record()
                    torch.cuda.synchronize()
                    if rep >= a.warmup:
                        ms[r].append(e0.elapsed_time(e1))
                    if rep == a.warmup + a.reps - 1:
                        flagged[r] = float((adj != 0).double().mean())
            case = dict(n=tpl.n, m=tpl.m, cones=cones, B=B, K=K, variant=variant, lds_bytes=lds, chunk=chunk, resident_workgroups_per_cu=cx["occ"], solved_share_of_base=cx["solved"] / BASE_B,
                        ms={r: stats(v) for r, v in ms.items()}, pairs_per_s={r: K * B / (np.median(v) * 1e-3) for r, v in ms.items()}, flagged_share=flagged)
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            dump()
            del dA, dq, dP

    sweep(BATCHES[0])
    if not a.skip_layer and over():
        res["not_measured"].append("layer"); dump()
    elif not a.skip_layer:
        from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
        from cvxpylayers_amd.torch.templates import template_from_affine_builder
        n, B = 16, 4096

        def builder(v, lo, hi):          # min 1/2 |x - v|^2, lo <= x <= hi
            return np.concatenate([-np.eye(n), np.eye(n)]), np.concatenate([-lo, hi]), -v, np.eye(n)
        layer = CvxpyLayer(template=template_from_affine_builder(builder, [(n,), (n,), (n,)], {"z": 0, "l": 2 * n, "q": [], "s": []}, [VariableRecovery(slice(0, n), None, (n,))]),
                           solver_args={"eps": 1e-8, "max_iters": 20000})
        rng = np.random.default_rng(SEED)
        ps = [torch.from_numpy(t).to(dev) for t in (rng.standard_normal((B, n)), -0.5 - 0.5 * rng.random((B, n)), 0.5 + 0.5 * rng.random((B, n)))]
        ms = {key: [] for key in LAYER_KEYS}
        for rep in range(a.warmup + a.reps):
            for key in (list(ms) if rep % 2 == 0 else list(ms)[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                layer.jacobian(*ps, solver_args=LAYER_KEYS[key], direction="reverse")
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    ms[key].append((time.perf_counter() - t0) * 1e3)
                assert layer.info["adjoint"]["path"] == ("ce_vjp_qp_many_wave" if "adjoint_kernel" in LAYER_KEYS[key] else "ce_vjp_qp_many")
        res["layer"] = dict(n=n, m=2 * n, B=B, eps=1e-8, what="box projection: jacobian(direction='reverse') (forward solve included), parameters (v, lo, hi), wall ms",
                            ms={k: stats(v) for k, v in ms.items()})
        print(json.dumps(res["layer"]), flush=True)
        dump()
    for B in BATCHES[1:]:
        sweep(B)


if __name__ == "__main__":
    main()
