"""Time of the many-tangent wave forward derivative (ce_jvp_many_wave, k_jvp_wave_many) against the ordinary many-tangent route (ce_jvp_many) and against K calls of
the single-tangent wave forward derivative (ce_jvp_wave) on small templates, one job, one box (profiles/jvp_wave_many/jvp_wave_many.json).

  families: scripts/fwd_wave_timing.py's seeded shapes (n, m) = (2, 3), (8, 16), (16, 32), (32, 64); points from the eps 1e-8 forward of the base batch, tiled to
            B = 4096 and 65536; K = n Gaussian tangents (tA and tq), "per_instance" = (K, B, .) tangents, "shared" = (K, .) tangents with batch stride 0 (what
            layer.jacobian(direction="forward") hands over); one output buffer shared by the routes.
  routes: "many_wave" = ce_jvp_many_wave, "many" = ce_jvp_many of this build, "k_wave" = K calls of ce_jvp_wave (per-instance tangents only: the entry takes no
          batch stride of 0), "parent" = ce_jvp_many of the parent commit's library (--parent-so: loaded beside this one's); alternating inside every repetition,
          HIP events around the call (the LSQR re-solve launch is part of every route), medians of --reps with min - max.
  per case: the row, its chunk, LDS and resident workgroups per CU (ce_jvp_wave_many_occupancy), the share of flagged pairs, at the first batch size the largest
            difference of dx, dy, ds between many_wave and many on the unflagged pairs.
  layer: layer.jacobian(direction="forward") at (16, 32), B = 4096, eps 1e-4, parameters (A, b, c), with and without newton_kernel="wave"; wall ms.

    python scripts/jvp_wave_many_timing.py [--reps 30] [--warmup 3] [--parent-so PATH] [--out profiles/jvp_wave_many/jvp_wave_many.json] [--skip-layer] [--budget-s S]
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

MANY_SHAPES = [SHAPES[i] for i in (0, 2, 3, 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-so", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jvp_wave_many", "jvp_wave_many.json"))
    ap.add_argument("--skip-layer", action="store_true")
    ap.add_argument("--budget-s", type=float, default=0.0, help="> 0: a case that would start after this many seconds is not measured (listed under not_measured)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    parent = Parent(a.parent_so) if a.parent_so else None
    if parent:
        parent.L.ce_jvp_many.argtypes = L.ce_jvp_many.argtypes
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
    i32 = dict(dtype=torch.int32, device=dev)
    ctxs = []
    for n, cones in MANY_SHAPES:
        tpl = P.dense_template(n, cones)
        A, b, c = P.generate(n, cones, BASE_B, seed=SEED)
        A_eval, q_eval = tpl.values_from_dense(A, b, c)
        eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, cones, dev)
        A0, q0 = torch.from_numpy(np.ascontiguousarray(A_eval.T)).to(dev), torch.from_numpy(q_eval).to(dev)
        x, y, s, _, status, _ = eng.solve(A0, q0, make_settings(dict(eps=1e-8, max_iters=20000)))
        gen = torch.Generator(device=dev).manual_seed(SEED + 1)
        ctxs.append(dict(tpl=tpl, cones=cones, eng=eng, hp=parent.create(tpl) if parent else None, occ=int(L.ce_jvp_wave_many_occupancy(eng._h)), A0=A0, q0=q0, pt=(x, y, s),
                         tan=(torch.randn((n, BASE_B, tpl.nnz_aug), generator=gen, **f64), torch.randn((n, BASE_B, n + 1), generator=gen, **f64))))

    def sweep(B, compare):
        for cx in ctxs:
            for tangents in ("per_instance", "shared"):
                tpl, cones, eng, hp = cx["tpl"], cx["cones"], cx["eng"], cx["hp"]
                n, m, nnz, K = tpl.n, tpl.m, tpl.nnz_aug, tpl.n
                if over():
                    res["not_measured"].append(dict(n=n, m=m, B=B, tangents=tangents)); dump()
                    continue
                variant, lds, chunk = eng.jvp_wave_many_plan()
                k = B // BASE_B
                A_bm = cx["A0"].repeat(k, 1).contiguous(); q_t = cx["q0"].repeat(1, k).contiguous()
                x, y, s = (t.repeat(k, 1).contiguous() for t in cx["pt"])
                if tangents == "shared":
                    tA, tq = (t[:, 0].contiguous() for t in cx["tan"]); sAb, sqb = 0, 0
                else:
                    tA, tq = (t.repeat(1, k, 1).contiguous() for t in cx["tan"]); sAb, sqb = nnz, n + 1
                dx, dy, ds = torch.empty((K, B, n), **f64), torch.empty((K, B, m), **f64), torch.empty((K, B, m), **f64)
                st, its = torch.empty((K, B), **i32), torch.empty((K, B), **i32)
                rule = (1e-8, 1e-8, 1e8, 0)

                def many(fn, h):
                    rc = fn(h, B, K, A_bm.data_ptr(), nnz, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), x.data_ptr(), y.data_ptr(), s.data_ptr(), tA.data_ptr(), tA.stride(0), sAb,
                            tq.data_ptr(), tq.stride(0), sqb, dx.data_ptr(), dy.data_ptr(), ds.data_ptr(), st.data_ptr(), its.data_ptr(), *rule, stream)
                    assert rc == 0, L.ce_last_error()

                def k_wave():
                    for kk in range(K):
                        rc = L.ce_jvp_wave(eng._h, B, A_bm.data_ptr(), nnz, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), x.data_ptr(), y.data_ptr(), s.data_ptr(), tA[kk].data_ptr(), nnz,
                                           tq[kk].data_ptr(), 1, n + 1, dx[kk].data_ptr(), dy[kk].data_ptr(), ds[kk].data_ptr(), st[kk].data_ptr(), its[kk].data_ptr(), *rule, stream)
                        assert rc == 0, L.ce_last_error()
                routes = [("many_wave", lambda: many(L.ce_jvp_many_wave, eng._h)), ("many", lambda: many(L.ce_jvp_many, eng._h))]
                if tangents == "per_instance":
                    routes.append(("k_wave", k_wave))
                if parent:
                    routes.append(("parent", lambda: many(parent.L.ce_jvp_many, hp)))
                ms = {r: [] for r, _ in routes}
                for rep in range(a.warmup + a.reps):
                    for r, fn in routes:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        e0.record(); fn(); e1.record()
                        torch.cuda.synchronize()
                        if rep >= a.warmup:
                            ms[r].append(e0.elapsed_time(e1))
                flagged, diff = {}, None
                for r, fn in routes[:2]:          # (one more call each for what the shared buffers hold)
                    fn(); torch.cuda.synchronize()
                    flagged[r] = float((st != 0).double().mean())
                    if compare and r == "many_wave":
                        keep, keep_st = [t.clone() for t in (dx, dy, ds)], st.clone()
                    elif compare:
                        clean = (keep_st == 0) & (st == 0)
                        rel = torch.stack([(g - w).abs().amax(dim=2) / (1 + w.abs().amax(dim=2)) for g, w in zip(keep, (dx, dy, ds))]).amax(dim=0)
                        diff = float(rel[clean].max()) if bool(clean.any()) else None
                        del keep
                case = dict(n=n, m=m, cones=cones, B=B, K=K, tangents=tangents, variant=variant, chunk=chunk, lds_bytes=lds, resident_workgroups_per_cu=cx["occ"],
                            ms={r: stats(v) for r, v in ms.items()}, pairs_per_s={r: K * B / (np.median(v) * 1e-3) for r, v in ms.items()},
                            flagged_share=flagged, max_rel_difference_many_wave_many_unflagged=diff)
                res["cases"].append(case)
                print(json.dumps(case), flush=True)
                dump()
                del tA, tq, dx, dy, ds, st, its
                torch.cuda.empty_cache()

    sweep(BATCHES[0], True)
    if not a.skip_layer and over():
        res["not_measured"].append("layer"); dump()
    elif not a.skip_layer:
        from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
        from cvxpylayers_amd.torch.templates import template_from_affine_builder
        n, cones = SHAPES[3]; m = P.cone_rows(cones); B = 4096
        layer = CvxpyLayer(template=template_from_affine_builder(lambda A, b, c: (A, b, c), [(m, n), (m,), (n,)], cones, [VariableRecovery(slice(0, n), None, (n,))]),
                           solver_args={"eps": 1e-4, "max_iters": 20000})
        ps = [torch.from_numpy(v).to(dev) for v in P.generate(n, cones, BASE_B, seed=SEED)]
        keys = {"none": {}, "newton": {"newton_kernel": "wave"}}
        ms = {key: [] for key in keys}
        for rep in range(a.warmup + a.reps):
            for key in ms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                layer.jacobian(*ps, solver_args=keys[key], direction="forward")
                torch.cuda.synchronize()
                if rep >= a.warmup:
                    ms[key].append((time.perf_counter() - t0) * 1e3)
                assert (layer.info["jvp"]["kernel"] == "ce_jvp_many_wave") == (key == "newton")
        res["layer"] = dict(n=n, m=m, cones=cones, B=B, eps=1e-4, tangents=m * n + m + n, what="layer.jacobian(direction='forward'), parameters (A, b, c), 16 outputs, wall ms",
                            ms={k: stats(v) for k, v in ms.items()})
        print(json.dumps(res["layer"]), flush=True)
        dump()
    for B in BATCHES[1:]:
        sweep(B, False)


if __name__ == "__main__":
    main()
