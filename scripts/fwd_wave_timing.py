"""Time of the one-instance-per-wave forward kernel (ce_solve_wave, k_fwd_wave) against the ordinary route (ce_solve) on small templates, one job, one box
(DESIGN.md section 3.23).  Per case the routes alternate repetition by repetition; HIP events around the call; medians of --reps after --warmup with min and max.

  shapes (n, m): (2, 3) l 3 | (4, 8) z 1, l 4, q [3] | (8, 16) z 2, l 6, q [3, 5] | (16, 32) z 2, l 10, q [4, 16] | (32, 64) z 4, l 20, q [8, 32]
  batches 4096 and 65536 (the seeded generator's 4096 instances, repeated 16 times for the larger batch: the same distribution of iteration counts)
  settings: eps 1e-4 with the default acceleration, eps 1e-8 without
  routes: "wave" = ce_solve_wave, "workgroup" = ce_solve of this build, "parent" = ce_solve of the parent commit's library (--parent-so: loaded beside this
  build's in the same process, so a drift of the box shows as a difference between "workgroup" and "parent")
Reported per case: instances / s of every route, the mean iteration counts and the largest per-instance difference of the counts between wave and
workgroup (a check interval at most without acceleration; a borderline safeguard decision may shift an accelerated instance), the instances not at status 1, the resident workgroups per CU of the instantiation (hipOccupancyMaxActiveBlocksPerMultiprocessor through ce_wave_occupancy).
Then a whole layer forward + backward of a scalar loss at (16, 32), B = 65536, under solver_args forward_kernel="wave" and without it (wall time, device idle
before and after).  Order: every shape at B = 4096, the layer, every shape at B = 65536; the JSON is rewritten after every case.

    python scripts/fwd_wave_timing.py [--reps 30] [--warmup 3] [--parent-so PATH] [--out profiles/fwd_wave/fwd_wave.json] [--skip-layer] [--budget-s S]
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

import torch  # noqa: E402

from cvxpylayers_amd import _lib  # noqa: E402
from cvxpylayers_amd import problems as P  # noqa: E402
from cvxpylayers_amd.interfaces.mi355_if import ConeEngine, make_settings  # noqa: E402

SHAPES = [(2, dict(z=0, l=3, q=[])), (4, dict(z=1, l=4, q=[3])), (8, dict(z=2, l=6, q=[3, 5])), (16, dict(z=2, l=10, q=[4, 16])), (32, dict(z=4, l=20, q=[8, 32]))]
BATCHES = (4096, 65536)
SETTINGS = (("eps1e-4_aa", dict(eps=1e-4, max_iters=20000)), ("eps1e-8_plain", dict(eps=1e-8, max_iters=20000, acceleration_lookback=0)))
BASE_B, SEED = 4096, 5


def stats(v):
    v = np.asarray(v, float)
    return dict(median=float(np.median(v)), min=float(v.min()), max=float(v.max()))


class Parent:
    """ce_create / ce_solve of another build of the library, loaded beside this one's"""

    def __init__(self, path):
        self.L = L = C.CDLL(path)
        vp, lg = C.c_void_p, C.c_long
        assert L.ce_abi_version() == _lib.ABI_VERSION
        L.ce_create.argtypes = [C.POINTER(_lib.CeTemplate), C.c_int, C.POINTER(vp)]
        L.ce_destroy.argtypes = [vp]
        L.ce_last_error.restype = C.c_char_p
        L.ce_solve.argtypes = [vp, C.c_int, vp, lg, lg, vp, lg, lg, C.POINTER(_lib.CeSettings), vp, vp, vp, vp, vp, vp, vp]

    def create(self, tpl):
        self.keep = q = np.ascontiguousarray(tpl.cones.get("q", []), dtype=np.int32)
        t = _lib.CeTemplate()
        t.n, t.m, t.nnz_aug = tpl.n, tpl.m, tpl.nnz_aug
        t.indices = tpl.indices.ctypes.data_as(C.POINTER(C.c_int)); t.indptr = tpl.indptr.ctypes.data_as(C.POINTER(C.c_int))
        t.z, t.l, t.nq, t.q = int(tpl.cones.get("z", 0)), int(tpl.cones.get("l", 0)), len(q), q.ctypes.data_as(C.POINTER(C.c_int))
        h = C.c_void_p()
        rc = self.L.ce_create(C.byref(t), 0, C.byref(h))
        assert rc == 0, self.L.ce_last_error()
        return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-so", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fwd_wave", "fwd_wave.json"))
    ap.add_argument("--skip-layer", action="store_true")
    ap.add_argument("--budget-s", type=float, default=0.0, help="> 0: a case that would start after this many seconds is not measured (listed under not_measured)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    L = _lib.lib()
    parent = Parent(a.parent_so) if a.parent_so else None
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
        A_eval, q_eval = tpl.values_from_dense(A, b, c)
        eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, cones, dev)
        ctxs.append(dict(tpl=tpl, cones=cones, eng=eng, hp=parent.create(tpl) if parent else None, occ=int(L.ce_wave_occupancy(eng._h)),
                         A0=torch.from_numpy(np.ascontiguousarray(A_eval.T)).to(dev), q0=torch.from_numpy(q_eval).to(dev)))

    def sweep(B):
        for cx in ctxs:
            tpl, cones, eng, hp = cx["tpl"], cx["cones"], cx["eng"], cx["hp"]
            variant, lds = eng.wave_plan()
            A_bm = cx["A0"].repeat(B // BASE_B, 1).contiguous(); q_t = cx["q0"].repeat(1, B // BASE_B).contiguous()
            out = dict(x=torch.empty((B, tpl.n), dtype=torch.float64, device=dev), y=torch.empty((B, tpl.m), dtype=torch.float64, device=dev),
                       s=torch.empty((B, tpl.m), dtype=torch.float64, device=dev), it=torch.empty((B,), dtype=torch.int32, device=dev),
                       st=torch.empty((B,), dtype=torch.int32, device=dev), r=torch.empty((B, 3), dtype=torch.float64, device=dev))
            for name, args in SETTINGS:
                if over():
                    res["not_measured"].append(dict(n=tpl.n, m=tpl.m, B=B, setting=name)); dump()
                    continue
                st = make_settings(dict(args))

                def call(fn, h):
                    rc = fn(h, B, A_bm.data_ptr(), 1, tpl.nnz_aug, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), C.byref(st), out["x"].data_ptr(), out["y"].data_ptr(),
                            out["s"].data_ptr(), out["it"].data_ptr(), out["st"].data_ptr(), out["r"].data_ptr(), stream)
                    assert rc == 0
                routes = [("wave", lambda: call(L.ce_solve_wave, eng._h)), ("workgroup", lambda: call(L.ce_solve, eng._h))]
                if parent:
                    routes.append(("parent", lambda: call(parent.L.ce_solve, hp)))
                ms = {k: [] for k, _ in routes}; iters = {}; unsolved = {}
                for rep in range(a.warmup + a.reps):
                    for k, fn in routes:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        e0.record(); fn(); e1.record()
                        torch.cuda.synchronize()
                        if rep >= a.warmup:
                            ms[k].append(e0.elapsed_time(e1))
                        if rep == 0:
                            iters[k] = out["it"].cpu().numpy().astype(int)
                            unsolved[k] = int((out["st"].cpu().numpy() != 1).sum())
                case = dict(n=tpl.n, m=tpl.m, cones=cones, B=B, setting=name, variant=variant, lds_bytes=lds, resident_workgroups_per_cu=cx["occ"],
                            ms={k: stats(v) for k, v in ms.items()}, instances_per_s={k: B / (np.median(v) * 1e-3) for k, v in ms.items()},
                            mean_iters={k: float(v.mean()) for k, v in iters.items()}, max_iters={k: int(v.max()) for k, v in iters.items()},
                            max_iters_difference_wave_workgroup=int(np.abs(iters["wave"] - iters["workgroup"]).max()), not_status_1=unsolved)
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
                           solver_args={"eps": 1e-4, "max_iters": 20000})
        A, b, c = P.generate(n, cones, BASE_B, seed=SEED)
        ps = [torch.from_numpy(np.ascontiguousarray(np.tile(v, (B // BASE_B,) + (1,) * (v.ndim - 1)))).to(dev).requires_grad_(True) for v in (A, b, c)]
        ms = {"wave": [], "workgroup": []}

        def step(key):
            for p in ps:
                p.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            (x,) = layer(*ps, solver_args={"forward_kernel": "wave"} if key == "wave" else None)
            (x ** 2).sum().backward()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        for rep in range(a.warmup + a.reps):
            for key in ms:
                t = step(key)
                if rep >= a.warmup:
                    ms[key].append(t)
                if key == "wave":
                    assert layer.info["forward"]["kernel"] == "k_fwd_wave"
        res["layer"] = dict(n=n, m=m, cones=cones, B=B, eps=1e-4, what="forward + backward of sum(x^2), parameters (A, b, c), wall ms", ms={k: stats(v) for k, v in ms.items()})
        print(json.dumps(res["layer"]), flush=True)
        dump()
    for B in BATCHES[1:]:
        sweep(B)


if __name__ == "__main__":
    main()
