"""Time of K cotangents at one solution of a native QP template: ce_vjp_qp_many (the search-free elimination with P, one factorisation per instance,
ConeEngine.vjp_many(qp_many=True)) against K sequential ce_vjp_qp calls (the pivoting kernel, one factorisation per cotangent), one box.

BASELINE configuration 2 in native form (box QP, P inside the kernels) at the eps = 1e-8 point: B = 4096 with K = 1, 2, 8, and B = 1024 with K = 50 (the reverse
Jacobian's shape: one cotangent per output); then CvxpyLayer.jacobian whole at B = 1024 for config 2's layer with parameters b and q, and again with P as a third
parameter: reverse search-free (solver_args qp_adjoint="search_free") against the reverse loop against direction="forward".

Per case wall time with the device idle before the clock starts and after it stops, alternating per repetition:
  (a) K sequential ConeEngine.vjp(P_bm=) calls of ANOTHER BUILD of this repository (--parent TREE: a checkout of the parent commit with its library built),
      run by a child process that is asked for one measurement at a time -- omitted without --parent;
  (b) the same K sequential calls of this build;
  (c) this build's vjp_many(qp_many=True).
Outputs are allocated inside the clock in all three.  Medians of --reps after --warmup calls, with min and max, and the number of flagged instances of each route.
Prints one JSON line; --out also writes it.

    python scripts/vjp_qp_many_timing.py [--reps 30] [--warmup 5] [--parent TREE] [--out profiles/vjp_qp_many/vjp_qp_many_C2.json]
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
    ap.add_argument("--no-layer", action="store_true", help="skip the CvxpyLayer.jacobian comparisons")
    ap.add_argument("--layer-reps", type=int, default=3)
    ap.add_argument("--worker", action="store_true")          # (internal: serve single measurements of the tree in --tree over stdin / stdout)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    return ap.parse_args()


a = _args()
sys.path.insert(0, a.tree)

import torch  # noqa: E402

from cvxpylayers_amd import problems as P  # noqa: E402
from cvxpylayers_amd.interfaces.mi355_if import ConeEngine, make_settings  # noqa: E402

SEED, EPS = 11, 1e-8
CASES = ((4096, 1), (4096, 2), (4096, 8), (1024, 50))          # (B, K)


class Bench:
    """config 2 in native form at batch size B, solved by this build at eps 1e-8, and Gaussian cotangents"""

    def __init__(self, B):
        self.B = B
        self.dev = torch.device("cuda", 0)
        nx = P.CONFIGS["C2"]["n"]
        A, b, q, Pm, pst, pv = P.native_box_qp_batch(nx, B, seed=SEED)
        self.n, self.cones = nx, P.CONFIGS["C2"]["cones"]
        self.tpl = P.dense_template(nx, self.cones, pattern=(A != 0))
        self.eng = ConeEngine(self.tpl.indices, self.tpl.indptr, self.tpl.n, self.tpl.m, self.tpl.cones, self.dev, p_structure=pst[:2])
        A = np.broadcast_to(A, (B,) + A.shape).copy()
        self.P_bm = torch.from_numpy(np.broadcast_to(pv, (B, pv.size)).copy()).to(self.dev)
        A_eval, q_eval = self.tpl.values_from_dense(A, b, q)
        self.A_bm = torch.from_numpy(np.ascontiguousarray(A_eval.T)).to(self.dev); self.q_t = torch.from_numpy(q_eval).to(self.dev)
        self.pt = tuple(self.eng.solve(self.A_bm, self.q_t, make_settings({"eps": EPS, "max_iters": 100000}), P_bm=self.P_bm)[:3])
        self._cot = {}

    def cotangents(self, K):
        if K not in self._cot:
            g = torch.Generator(device="cpu").manual_seed(SEED + K)
            self._cot[K] = tuple(torch.randn((K, self.B, w), generator=g, dtype=torch.float64).to(self.dev) for w in (self.n, self.tpl.m))
        return self._cot[K]

    def sequential(self, K):
        """K ce_vjp_qp calls: (wall ms, flagged instances)"""
        dx, dy = self.cotangents(K)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = [self.eng.vjp(self.A_bm, *self.pt, dx[k], dy[k], P_bm=self.P_bm, path="per_instance") for k in range(K)]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, int((outs[0][2] != 0).sum())

    def many(self, K):
        dx, dy = self.cotangents(K)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = self.eng.vjp_many(self.A_bm, *self.pt, dx, dy, path="per_instance", P_bm=self.P_bm, qp_many=True)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        assert self.eng.last_vjp_many_path == "many" and self.eng.last_vjp_kernel == "ce_vjp_qp_many"
        return ms, int((out[2][0] != 0).sum())


def worker():
    benches = {}
    print("ready", flush=True)
    for line in sys.stdin:
        req = json.loads(line)
        if req["B"] not in benches:
            benches[req["B"]] = Bench(req["B"])
        ms, fl = benches[req["B"]].sequential(req["K"])
        print(json.dumps({"ms": ms, "flagged": fl}), flush=True)


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def _layer(with_P, B):
    from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
    from cvxpylayers_amd.torch.templates import template_from_affine_builder
    nx = P.CONFIGS["C2"]["n"]
    A, b, q, Pm, _, _ = P.native_box_qp_batch(nx, B, seed=SEED)
    cones, rec = {"z": 0, "l": 2 * nx, "q": [], "s": []}, [VariableRecovery(slice(0, nx), None, (nx,))]
    if with_P:
        tpl = template_from_affine_builder(lambda Pp, bv, qv: (A, bv, qv, 0.5 * (Pp + Pp.T)), [(nx, nx), (2 * nx,), (nx,)], cones, rec)
        params = [torch.from_numpy(np.broadcast_to(Pm, (B, nx, nx)).copy()).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(q).cuda()]
        what = "config 2's layer with P (50 x 50) as a parameter beside b and q, A constant; x is the output"
    else:
        tpl = template_from_affine_builder(lambda bv, qv: (A, bv, qv, Pm), [(2 * nx,), (nx,)], cones, rec)
        params = [torch.from_numpy(b).cuda(), torch.from_numpy(q).cuda()]
        what = "config 2's layer: parameters b (the bounds) and q, P and A constant; x is the output"
    return CvxpyLayer(template=tpl, solver_args={"eps": EPS, "max_iters": 100000}), params, nx, tpl.n_params_total, what


ROUTES = (("reverse_search_free", dict(direction="reverse", solver_args={"qp_adjoint": "search_free"})), ("reverse_loop", dict(direction="reverse")),
          ("forward", dict(direction="forward")))


def layer_jacobian(with_P, reps, B=1024):
    """CvxpyLayer.jacobian whole on the three routes, alternating; each includes the forward solve"""
    layer, params, n_out, n_par, what = _layer(with_P, B)
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    t, paths, flagged, err = {k: [] for k, _ in ROUTES}, {}, {}, {}
    for it in range(1 + reps):
        jac = {}
        for key, kw in ROUTES:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            _, jac[key] = layer.jacobian(*params, **kw)
            torch.cuda.synchronize(); ms = (time.perf_counter() - t0) * 1e3
            paths[key] = eng.last_jvp_many_path if key == "forward" else eng.last_vjp_many_path
            st = layer.info["jvp" if key == "forward" else "adjoint"]["status"]
            flagged[key] = int((st[0] != 0).sum())
            if it >= 1:
                t[key].append(ms)
        for key in ("reverse_search_free", "forward"):
            err[key + "_against_reverse_loop"] = max(float((f - r).abs().max() / (1 + r.abs().max())) for f, r in zip(jac[key][0], jac["reverse_loop"][0]))
        del jac
    return {"B": B, "outputs": n_out, "parameter_entries": n_par, "reps": reps, "layer": what, "wall_ms": {k: stat(v) for k, v in t.items()}, "paths": paths,
            "flagged": flagged, **err}


def main():
    benches = {B: Bench(B) for B in sorted({B for B, _ in CASES})}
    child = None
    if a.parent:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--tree", os.path.abspath(a.parent)],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=os.path.abspath(a.parent))
        assert child.stdout.readline().strip() == "ready"
    rows = []
    for B, K in CASES:
        bench = benches[B]
        t = {"a_parent_sequential": [], "b_sequential": [], "c_many": []}
        fl = {}
        for it in range(a.warmup + a.reps):
            if child is not None:
                child.stdin.write(json.dumps({"B": B, "K": K}) + "\n"); child.stdin.flush()
                r = json.loads(child.stdout.readline())
                fl["a_parent_sequential"] = r["flagged"]
                if it >= a.warmup:
                    t["a_parent_sequential"].append(r["ms"])
            for key, fn in (("b_sequential", bench.sequential), ("c_many", bench.many)):
                ms, fl[key] = fn(K)
                if it >= a.warmup:
                    t[key].append(ms)
        st = {k_: stat(v) for k_, v in t.items() if v}
        row = {"B": B, "K": K, "wall_ms": st, "per_cotangent_ms": {k_: v["median"] / K for k_, v in st.items()}, "flagged": fl}
        ref = st.get("a_parent_sequential", st["b_sequential"])
        row["many_bracket_below_sequential"] = st["c_many"]["max"] < ref["min"]
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    if child is not None:
        child.stdin.close(); child.wait(timeout=60)
    b0 = benches[CASES[0][0]]
    res = {"config": "C2", "eps": EPS, "n": b0.n, "m": b0.tpl.m, "nnz_aug": b0.tpl.nnz_aug, "nnz_p": b0.eng.nnz_p, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "parent": bool(a.parent), "rows": rows}
    del benches
    if not a.no_layer:
        for key, with_P in (("layer_jacobian_b_q", False), ("layer_jacobian_P_b_q", True)):
            try:
                res[key] = layer_jacobian(with_P, a.layer_reps)
            except Exception as e:          # (a record of the calls is worth keeping when a layer comparison fails)
                res[key] = {"error": f"{type(e).__name__}: {e}"}
            print(json.dumps({key: res[key]}), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    worker() if a.worker else main()
