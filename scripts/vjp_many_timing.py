"""Time of K cotangents at one solution: ce_vjp_many (one factorisation per instance, ConeEngine.vjp_many) against K sequential ce_vjp calls, at the metric
configuration and the eps = 1e-8 point, one box.

Per case (B, K) -- (4096, 1), (4096, 2), (4096, 8) and (1024, 50), the full Jacobian of the metric shape's x -- wall time with the device idle before the clock
starts and after it stops, alternating per repetition:
  (a) K sequential ConeEngine.vjp calls of ANOTHER BUILD of this repository (--parent TREE: a checkout of the parent commit with its library built), run by a child
      process that is asked for one measurement at a time -- omitted without --parent;
  (b) the same K sequential calls of this build (vjp_many(force_loop=True) without its stacking: the calls alone);
  (c) this build's vjp_many.
Outputs are allocated inside the clock in all three (each call returns fresh tensors).  Then the bytes-written rate of (c)'s dA stream (K B nnz_aug 8 bytes over its
median) beside ce_transpose of an array of the same size in the same run, and the flagged count.  Last, CvxpyLayer.jacobian whole at B = 1024 (a layer whose
parameters are A, b and c of the metric shape) against the loop of torch.autograd.grad over one-hot cotangents it replaces.  Medians of --reps after --warmup
calls, with min and max.  Prints one JSON line; --out also writes it.

    python scripts/vjp_many_timing.py [--reps 30] [--warmup 5] [--parent TREE] [--out profiles/vjp_many/vjp_many_M.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np


def _args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-layer", action="store_true", help="skip the CvxpyLayer.jacobian comparison")
    ap.add_argument("--worker", action="store_true")          # (internal: serve single measurements of the tree in --tree over stdin / stdout)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    return ap.parse_args()


a = _args()
sys.path.insert(0, a.tree)

import torch  # noqa: E402

from cvxpylayers_amd import problems as P  # noqa: E402
from cvxpylayers_amd.interfaces.mi355_if import ConeEngine, make_settings  # noqa: E402

SEED, EPS = 11, 1e-8
CASES = ((4096, 1), (4096, 2), (4096, 8), (1024, 50))


class Bench:
    """the metric batch of one build, solved by that build at eps 1e-8, and Gaussian cotangents"""

    def __init__(self):
        cfg = P.CONFIGS["M"]
        self.n, self.cones = cfg["n"], cfg["cones"]
        self.tpl = P.dense_template(self.n, self.cones)
        self.dev = torch.device("cuda", 0)
        self.eng = ConeEngine(self.tpl.indices, self.tpl.indptr, self.tpl.n, self.tpl.m, self.tpl.cones, self.dev)
        self._pt, self._cot = {}, {}

    def point(self, B):
        if B not in self._pt:
            A, b, c = P.generate(self.n, self.cones, B, seed=SEED)
            A_eval, q_eval = self.tpl.values_from_dense(A, b, c)
            A_bm = torch.from_numpy(np.ascontiguousarray(A_eval.T)).to(self.dev); q_t = torch.from_numpy(q_eval).to(self.dev)
            x, y, s, *_ = self.eng.solve(A_bm, q_t, make_settings({"eps": EPS, "max_iters": 100000}))
            self._pt[B] = (A_bm, q_t, x, y, s)
        return self._pt[B]

    def cot(self, B, K):
        if (B, K) not in self._cot:
            g = torch.Generator(device="cpu").manual_seed(SEED + K)
            self._cot[(B, K)] = (torch.randn((K, B, self.n), generator=g, dtype=torch.float64).to(self.dev), torch.randn((K, B, self.tpl.m), generator=g, dtype=torch.float64).to(self.dev))
        return self._cot[(B, K)]

    def sequential(self, B, K):
        """K ce_vjp calls: (wall ms, flagged instances of the first)"""
        A_bm, q_t, x, y, s = self.point(B)
        dx, dy = self.cot(B, K)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = [self.eng.vjp(A_bm, x, y, s, dx[k], dy[k], path="per_instance", q_eval=q_t) for k in range(K)]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, int((outs[0][2] != 0).sum())

    def many(self, B, K):
        A_bm, q_t, x, y, s = self.point(B)
        dx, dy = self.cot(B, K)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = self.eng.vjp_many(A_bm, x, y, s, dx, dy, path="per_instance", q_eval=q_t)
        torch.cuda.synchronize()
        assert self.eng.last_vjp_many_path == "many"
        return (time.perf_counter() - t0) * 1e3, int((out[2][0] != 0).sum())

    def transpose(self, rows, cols):
        src = torch.empty((cols, rows), dtype=torch.float64, device=self.dev).normal_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        self.eng.to_batch_major(src)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3


def worker():
    bench = Bench()
    print("ready", flush=True)
    for line in sys.stdin:
        req = json.loads(line)
        ms, fl = bench.sequential(req["B"], req["K"])
        print(json.dumps({"ms": ms, "flagged": fl}), flush=True)


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def layer_jacobian(reps):
    """CvxpyLayer.jacobian whole against the autograd loop it replaces: a layer with parameters (A, b, c) of the metric shape, x as the output, B = 1024"""
    from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
    from cvxpylayers_amd.torch.templates import template_from_affine_builder
    cfg = P.CONFIGS["M"]
    n, cones, B = cfg["n"], cfg["cones"], 1024
    m = P.cone_rows(cones)
    tpl = template_from_affine_builder(lambda A, b, c: (A, b, c), [(m, n), (m,), (n,)], cones, [VariableRecovery(slice(0, n), None, (n,))])
    layer = CvxpyLayer(template=tpl, solver_args={"eps": EPS, "max_iters": 100000})
    params = [torch.from_numpy(t).cuda() for t in P.generate(n, cones, B, seed=SEED)]
    t_j, t_l = [], []
    for it in range(1 + reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        outs, jac = layer.jacobian(*params)
        torch.cuda.synchronize(); tj = (time.perf_counter() - t0) * 1e3
        del jac
        ps = [p.clone().requires_grad_(True) for p in params]
        torch.cuda.synchronize(); t0 = time.perf_counter()
        (x,) = layer(*ps)
        rows = []
        for t in range(n):
            oh = torch.zeros_like(x); oh[:, t] = 1.0
            rows.append(torch.autograd.grad(x, ps, grad_outputs=oh, retain_graph=True))
        torch.cuda.synchronize(); tl = (time.perf_counter() - t0) * 1e3
        del rows
        if it >= 1:
            t_j.append(tj); t_l.append(tl)
    return {"B": B, "outputs": n, "parameter_entries": tpl.n_params_total, "reps": reps, "jacobian_ms": stat(t_j), "autograd_loop_ms": stat(t_l),
            "note": "both include the forward solve; the autograd loop is one layer call and 50 torch.autograd.grad calls on its graph"}


def main():
    bench = Bench()
    child = None
    if a.parent:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--tree", os.path.abspath(a.parent)],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=os.path.abspath(a.parent))
        assert child.stdout.readline().strip() == "ready"
    K_aug = bench.tpl.nnz_aug
    rows = []
    for B, K in CASES:
        t = {"a_parent_sequential": [], "b_sequential": [], "c_many": [], "ce_transpose_same_bytes": []}
        fl = {}
        for it in range(a.warmup + a.reps):
            if child is not None:
                child.stdin.write(json.dumps({"B": B, "K": K}) + "\n"); child.stdin.flush()
                r = json.loads(child.stdout.readline())
                fl["a_parent_sequential"] = r["flagged"]
                if it >= a.warmup:
                    t["a_parent_sequential"].append(r["ms"])
            for key, fn in (("b_sequential", bench.sequential), ("c_many", bench.many)):
                ms, fl[key] = fn(B, K)
                if it >= a.warmup:
                    t[key].append(ms)
            ms = bench.transpose(K * B, K_aug)
            if it >= a.warmup:
                t["ce_transpose_same_bytes"].append(ms)
        st = {k_: stat(v) for k_, v in t.items() if v}
        nbytes = 8.0 * K * B * K_aug
        row = {"B": B, "K": K, "wall_ms": st, "per_cotangent_ms": {k_: v["median"] / K for k_, v in st.items() if k_ != "ce_transpose_same_bytes"}, "flagged": fl,
               "dA_bytes": nbytes, "dA_GB_per_s_many": nbytes / (st["c_many"]["median"] * 1e-3) / 1e9,
               "transpose_GB_per_s_written": nbytes / (st["ce_transpose_same_bytes"]["median"] * 1e-3) / 1e9}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    if child is not None:
        child.stdin.close(); child.wait(timeout=60)
    res = {"config": "M", "eps": EPS, "n": bench.n, "m": bench.tpl.m, "nnz_aug": K_aug, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "parent": bool(a.parent), "rows": rows}
    if not a.no_layer:
        res["layer_jacobian"] = layer_jacobian(3)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    worker() if a.worker else main()
