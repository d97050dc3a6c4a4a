"""Time of the parameter gradient from the adjoint's factors (solver_args param_grad="factors") against the dA route, at the metric configuration and the
eps = 1e-8 point, one box.  Wall time with the device idle before the clock starts and after it stops, the routes alternating per repetition;
medians of --reps after --warmup with min and max.

  (a) engine level, (B, K) = (4096, 8) and (1024, 50): ConeEngine.vjp_many_params against vjp_many plus the two transposed-map products, for the maps of a layer
      with parameters (A, b, c) -- Ptot = 5150 -- and of one with (b, c) -- 150;
  (b) CvxpyLayer.jacobian(direction="reverse") whole, B = 1024, K = 50 outputs, both parameter sets: the key against the default;
  (c) a whole layer forward + backward of a scalar loss, B = 4096, both parameter sets: the key against the default.
With --parent TREE (a checkout of the parent commit with its library built) a child process serves the DEFAULT route of that build for every case, one measurement
at a time, alternating with this build's.  For the new kernel alone: its algorithmic bytes (factor records and dq read, x and y read, g written), the rate reached
(the kernel is timed by the events the engine puts around it under ce_set_profiling: its profile slot 2), and ce_transpose on an array of g's size in the same run.  No instance may be flagged (asserted).

    python scripts/param_grad_timing.py [--reps 30] [--warmup 5] [--parent TREE] [--out profiles/param_grad/param_grad_M.json]
"""
import argparse
import ctypes as C
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
    ap.add_argument("--kernel-only", action="store_true", help="the engine-level cases' k_param_grad block alone (events around the kernel, ce_transpose of g's size)")
    ap.add_argument("--worker", action="store_true")          # (internal: serve single measurements of the tree in --tree over stdin / stdout)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    return ap.parse_args()


a = _args()
sys.path.insert(0, a.tree)

import torch  # noqa: E402

from cvxpylayers_amd import _lib  # noqa: E402
from cvxpylayers_amd import problems as P  # noqa: E402
from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery  # noqa: E402
from cvxpylayers_amd.torch.cvxpylayer import _spmm_bm  # noqa: E402
from cvxpylayers_amd.torch.templates import template_from_affine_builder  # noqa: E402

SEED, EPS = 11, 1e-8
ENGINE_CASES = ((4096, 8), (1024, 50))
KEY = {"param_grad": "factors"}


def sync_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


class Bench:
    """the two layers of the metric shape in one build, their batches solved by that build at eps 1e-8"""

    def __init__(self):
        cfg = P.CONFIGS["M"]
        self.n, self.cones = cfg["n"], cfg["cones"]
        n, cones = self.n, self.cones
        self.m = m = P.cone_rows(cones)
        rec = [VariableRecovery(slice(0, n), None, (n,))]
        A0 = P.generate(n, cones, 1, seed=SEED, batched=("b", "c"))[0][0]          # (the generator draws the shared A first: the same for every B)
        self.layers = {
            "Abc": CvxpyLayer(template=template_from_affine_builder(lambda A, b, c: (A, b, c), [(m, n), (m,), (n,)], cones, rec), solver_args={"eps": EPS, "max_iters": 100000}),
            "bc": CvxpyLayer(template=template_from_affine_builder(lambda b, c: (A0, b, c), [(m,), (n,)], cones, rec), solver_args={"eps": EPS, "max_iters": 100000}),
        }
        self.dev = torch.device("cuda", 0)
        self._params, self._pt, self._cot = {}, {}, {}

    def params(self, kind, B):
        if (kind, B) not in self._params:
            A, b, c = P.generate(self.n, self.cones, B, seed=SEED, batched=("A", "b", "c") if kind == "Abc" else ("b", "c"))
            ps = (A, b, c) if kind == "Abc" else (b, c)
            self._params[(kind, B)] = [torch.from_numpy(np.ascontiguousarray(t)).to(self.dev) for t in ps]
        return self._params[(kind, B)]

    # ---- (a) engine level: the point of the "Abc" layer's batch, Gaussian cotangents
    def point(self, B):
        if B not in self._pt:
            layer = self.layers["Abc"]
            with torch.no_grad():
                layer(*self.params("Abc", B))
            eng = layer.ctx.solver_ctx.engine(self.dev)
            A, b, c = P.generate(self.n, self.cones, B, seed=SEED)
            tpl = P.dense_template(self.n, self.cones)
            A_eval, q_eval = tpl.values_from_dense(A, b, c)
            A_bm = torch.from_numpy(np.ascontiguousarray(A_eval.T)).to(self.dev); q_t = torch.from_numpy(q_eval).to(self.dev)
            from cvxpylayers_amd.interfaces.mi355_if import make_settings
            x, y, s, *_ = eng.solve(A_bm, q_t, make_settings({"eps": EPS, "max_iters": 100000}))
            self._pt[B] = (eng, A_bm, q_t, x, y, s)
        return self._pt[B]

    def cot(self, B, K):
        if (B, K) not in self._cot:
            g = torch.Generator(device="cpu").manual_seed(SEED + K)
            self._cot[(B, K)] = (torch.randn((K, B, self.n), generator=g, dtype=torch.float64).to(self.dev), torch.randn((K, B, self.m), generator=g, dtype=torch.float64).to(self.dev))
        return self._cot[(B, K)]

    def engine_default(self, kind, B, K):
        eng, A_bm, q_t, x, y, s = self.point(B)
        dx, dy = self.cot(B, K)
        layer = self.layers[kind]
        bA, bq = layer._A.on(self.dev)[1], layer._q.on(self.dev)[1]
        def run():
            dA, dq, adj = eng.vjp_many(A_bm, x, y, s, dx, dy, path="per_instance", q_eval=q_t)
            g = torch.empty((K * B, bA[3]), dtype=torch.float64, device=self.dev)
            _spmm_bm(bA, dA.view(K * B, -1), out=g.zero_())
            _spmm_bm(bq, dq.view(K * B, -1), out=g)
            return adj
        ms, adj = sync_ms(run)
        return ms, int((adj != 0).sum())

    def engine_factors(self, kind, B, K):
        eng, A_bm, q_t, x, y, s = self.point(B)
        dx, dy = self.cot(B, K)
        maps = self.layers[kind]._pg_maps()
        ms, out = sync_ms(lambda: eng.vjp_many_params(A_bm, x, y, s, dx, dy, maps, q_eval=q_t))
        return ms, int((out[2] != 0).sum())

    def kernel_alone(self, kind, B, K):
        """the map stage of the last vjp_many_params call alone, from the engine's profile slot 2 (events around k_param_grad), ms"""
        eng, A_bm, q_t, x, y, s = self.point(B)
        dx, dy = self.cot(B, K)
        maps = self.layers[kind]._pg_maps()
        L = _lib.lib()
        L.ce_reset_profile(eng._h); L.ce_set_profiling(eng._h, 8)          # (8: the layout scope alone -- slot 2, where k_param_grad is bracketed)
        eng.vjp_many_params(A_bm, x, y, s, dx, dy, maps, q_eval=q_t)
        torch.cuda.synchronize()
        tot, cnt = C.c_double(), C.c_int()
        L.ce_get_profile(eng._h, 2, C.byref(tot), C.byref(cnt))
        L.ce_set_profiling(eng._h, 0); L.ce_reset_profile(eng._h)
        return tot.value / max(1, cnt.value)

    def transpose(self, rows, cols):
        eng = self.point(1024)[0]
        src = torch.empty((cols, rows), dtype=torch.float64, device=self.dev).normal_()
        return sync_ms(lambda: eng.to_batch_major(src))[0]

    # ---- (b), (c): through the layer
    def jacobian(self, kind, key):
        ms, _ = sync_ms(lambda: self.layers[kind].jacobian(*self.params(kind, 1024), solver_args=KEY if key else None)[1][0][0].shape)
        return ms, int((self.layers[kind].info["adjoint"]["status"] != 0).sum())

    def step(self, kind, key):
        layer = self.layers[kind]
        ps = [p.detach().requires_grad_(True) for p in self.params(kind, 4096)]
        def run():
            (x,) = layer(*ps, solver_args=KEY if key else None)
            x.sum().backward()
        ms, _ = sync_ms(run)
        return ms, int((layer.info["adjoint"]["status"] != 0).sum())

    def measure(self, req):
        what, kind, key = req["what"], req["kind"], req.get("key", False)
        if what == "engine":
            return (self.engine_factors if key else self.engine_default)(kind, req["B"], req["K"])
        return (self.jacobian if what == "jacobian" else self.step)(kind, key)


def worker():
    bench = Bench()
    print("ready", flush=True)
    for line in sys.stdin:
        ms, fl = bench.measure(json.loads(line))
        print(json.dumps({"ms": ms, "flagged": fl}), flush=True)


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    bench = Bench()
    child = None
    if a.parent:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--tree", os.path.abspath(a.parent)],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=os.path.abspath(a.parent))
        assert child.stdout.readline().strip() == "ready"
    cases = [dict(what="engine", kind=k, B=B, K=K) for B, K in ENGINE_CASES for k in ("Abc", "bc")]
    cases += [dict(what="jacobian", kind=k, B=1024, K=50) for k in ("Abc", "bc")] + [dict(what="step", kind=k, B=4096, K=1) for k in ("Abc", "bc")]
    rows = []
    for case in cases:
        reps = a.reps if case["what"] != "jacobian" else max(5, a.reps // 3)          # (a whole Jacobian takes tens of milliseconds to seconds)
        t = {"parent_default": [], "default": [], "factors": []}
        if a.kernel_only and case["what"] != "engine":
            continue
        for it in range(0 if a.kernel_only else a.warmup + reps):
            if child is not None:
                child.stdin.write(json.dumps(case) + "\n"); child.stdin.flush()
                r = json.loads(child.stdout.readline())
                assert r["flagged"] == 0, (case, r)
                if it >= a.warmup:
                    t["parent_default"].append(r["ms"])
            for route, key in (("default", False), ("factors", True)):
                ms, fl = bench.measure({**case, "key": key})
                assert fl == 0, (case, route, fl)
                if it >= a.warmup:
                    t[route].append(ms)
        row = {**case, "reps": reps, "wall_ms": {k_: stat(v) for k_, v in t.items() if v}}
        if not a.kernel_only:
            row["factors_over_default"] = row["wall_ms"]["factors"]["median"] / row["wall_ms"]["default"]["median"]
        if case["what"] == "engine":
            B, K, kind = case["B"], case["K"], case["kind"]
            maps = bench.layers[kind]._pg_maps()
            n, m = bench.n, bench.m
            kern = [bench.kernel_alone(kind, B, K) for _ in range(a.warmup + reps)][a.warmup:]
            tr = [bench.transpose(K * B, maps.rows) for _ in range(a.warmup + reps)][a.warmup:]
            nbytes = 8.0 * K * B * ((m + 1 + n) + (n + 1) + maps.rows) + 8.0 * B * (n + m)
            row["k_param_grad"] = {"rows": maps.rows, "map_entries": int(maps.ptr[-1]), "event_ms": stat(kern), "algorithmic_bytes": nbytes,
                                   "GB_per_s": nbytes / (np.median(kern) * 1e-3) / 1e9, "g_bytes": 8.0 * K * B * maps.rows,
                                   "ce_transpose_same_size_ms": stat(tr), "ce_transpose_GB_per_s_written": 8.0 * K * B * maps.rows / (np.median(tr) * 1e-3) / 1e9}
        if case["what"] != "engine":
            adj = bench.layers[case["kind"]].info["adjoint"]
            row["route_of_the_last_call"] = {"path": adj.get("path"), "param_grad": adj.get("param_grad")}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    if child is not None:
        child.stdin.close(); child.wait(timeout=60)
    res = {"config": "M", "eps": EPS, "n": bench.n, "m": bench.m, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "parent": bool(a.parent), "rows": rows}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    worker() if a.worker else main()
