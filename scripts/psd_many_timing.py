"""Time of K cotangents and of K tangents at one solution of a template with PSD blocks: ce_vjp_psd_many / ce_jvp_psd_many (the search-free elimination with PSD
blocks, one decomposition, rotation and factorisation per instance, one LSQR launch for the flagged instances of every right-hand side;
ConeEngine.vjp_many / jvp_many(psd_many=True)) against K single calls of the routes they replace, one box.

Shape lqr_like (tests/psd_ns_kit.py: n = 24, 3 zero and 2 nonnegative rows, PSD blocks of order 6 and 4, m = 36) at the eps = 1e-8 point: B = 4096 with
K = 1, 2, 8, and B = 1024 with K = n = 24, the output count of the layer below; then CvxpyLayer.jacobian whole at B = 1024 in both directions for a layer on that
shape with parameters A, b and c and output x, with and without the keys psd_adjoint / psd_tangents.

Per case wall time with the device idle before the clock starts and after it stops, alternating per repetition:
  adjoint   (a) K sequential ConeEngine.vjp calls (ce_vjp: the pivoting kernel) of ANOTHER BUILD of this repository (--parent TREE: a checkout of the parent commit
                with its library built), run by a child process that is asked for one measurement at a time -- omitted without --parent;
            (b) the same K sequential calls of this build;  (c) this build's vjp_many(psd_many=True);
  forward   (a) K sequential ConeEngine.jvp(method="direct") calls of the parent build -- ce_jvp_lsqr, what jvp_many's loop runs on such a template -- and
            (a2) with psd_ns=True -- ce_jvp_psd;  (b), (b2) the same of this build;  (c) this build's jvp_many(psd_many=True).
All under the default re-solve rule with q_eval given; outputs are allocated inside the clock.  Medians of --reps after --warmup calls, with min and max, and the
share of flagged instances.  Prints one JSON line; --out also writes it.

    python scripts/psd_many_timing.py [--reps 30] [--warmup 5] [--parent TREE] [--out profiles/psd_many/psd_many_lqr_like.json]
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
    ap.add_argument("--layer-reps", type=int, default=3)
    ap.add_argument("--worker", action="store_true")          # (internal: serve single measurements of the tree in --tree over stdin / stdout)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    return ap.parse_args()


a = _args()
sys.path.insert(0, a.tree)

import torch  # noqa: E402

from cvxpylayers_amd import problems as P  # noqa: E402
from cvxpylayers_amd.interfaces.mi355_if import ConeEngine, make_settings  # noqa: E402

SEED, EPS = 3, 1e-8
N, CONES = 24, {"z": 3, "l": 2, "s": [6, 4]}          # tests/psd_ns_kit.py SHAPES["lqr_like"]
CASES = ((4096, 1), (4096, 2), (4096, 8), (1024, N))          # (B, K)


class Bench:
    """lqr_like at batch size B, solved by this build at eps 1e-8, and Gaussian right-hand sides"""

    def __init__(self, B):
        self.B = B
        self.dev = torch.device("cuda", 0)
        A, b, c = P.generate(N, CONES, B, seed=SEED)
        self.tpl = P.dense_template(N, CONES)
        self.eng = ConeEngine(self.tpl.indices, self.tpl.indptr, self.tpl.n, self.tpl.m, self.tpl.cones, self.dev)
        A_eval, q_eval = self.tpl.values_from_dense(A, b, c)
        self.A_bm = torch.from_numpy(np.ascontiguousarray(A_eval.T)).to(self.dev); self.q_t = torch.from_numpy(q_eval).to(self.dev)
        out = self.eng.solve(self.A_bm, self.q_t, make_settings({"eps": EPS, "max_iters": 100000}))
        self.pt = tuple(out[:3])
        self.unsolved = int((out[4] != 1).sum())
        self._rhs = {}

    def rhs(self, K):
        """dx (K, B, n), dy (K, B, m), tA (K, B, nnz_aug), tq (K, B, n + 1), drawn on the device"""
        if K not in self._rhs:
            g = torch.Generator(device=self.dev).manual_seed(SEED + K)
            self._rhs = {K: tuple(torch.randn((K, self.B, w), generator=g, dtype=torch.float64, device=self.dev) for w in (N, self.tpl.m, self.tpl.nnz_aug, N + 1))}
        return self._rhs[K]

    def _timed(self, fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, int((st != 0).sum())

    def vjp_sequential(self, K):
        dx, dy, _, _ = self.rhs(K)
        return self._timed(lambda: [self.eng.vjp(self.A_bm, *self.pt, dx[k], dy[k], path="per_instance", q_eval=self.q_t) for k in range(K)][0][2])

    def vjp_many(self, K):
        dx, dy, _, _ = self.rhs(K)
        r = self._timed(lambda: self.eng.vjp_many(self.A_bm, *self.pt, dx, dy, path="per_instance", q_eval=self.q_t, psd_many=True)[2][0])
        assert self.eng.last_vjp_kernel == "ce_vjp_psd_many"
        return r

    def jvp_sequential(self, K, psd_ns):
        _, _, tA, tq = self.rhs(K)
        r = self._timed(lambda: [self.eng.jvp(self.A_bm, *self.pt, tA[k], tq[k].t(), path="per_instance", q_eval=self.q_t, method="direct", psd_ns=psd_ns)
                                 for k in range(K)][0][3])
        assert self.eng.last_jvp_kernel == ("ce_jvp_psd" if psd_ns else "ce_jvp_lsqr")
        return r

    def jvp_many(self, K):
        _, _, tA, tq = self.rhs(K)
        r = self._timed(lambda: self.eng.jvp_many(self.A_bm, *self.pt, tA, tq, path="per_instance", q_eval=self.q_t, method="direct", psd_many=True)[3][0])
        assert self.eng.last_jvp_kernel == "ce_jvp_psd_many"
        return r

    def measure(self, what, K):
        return {"vjp_sequential": lambda: self.vjp_sequential(K), "vjp_many": lambda: self.vjp_many(K), "jvp_lsqr_sequential": lambda: self.jvp_sequential(K, False),
                "jvp_psd_sequential": lambda: self.jvp_sequential(K, True), "jvp_many": lambda: self.jvp_many(K)}[what]()

    def agreement(self, K):
        """largest relative difference between the one call and the loop on instances both report status 0, per direction"""
        dx, dy, tA, tq = self.rhs(K)
        kw = dict(path="per_instance", q_eval=self.q_t)
        m = self.eng.vjp_many(self.A_bm, *self.pt, dx, dy, psd_many=True, **kw); l = self.eng.vjp_many(self.A_bm, *self.pt, dx, dy, force_loop=True, **kw)
        both = (m[2] == 0) & (l[2] == 0)
        ev = max(float(((m[i] - l[i]).abs().amax(dim=2) / (1 + l[i].abs().amax(dim=2)))[both].max()) for i in range(2))
        m = self.eng.jvp_many(self.A_bm, *self.pt, tA, tq, psd_many=True, method="direct", **kw)
        l = self.eng.jvp_many(self.A_bm, *self.pt, tA, tq, psd_many=True, force_loop=True, method="direct", **kw)
        both = (m[3] == 0) & (l[3] == 0)
        ej = max(float(((m[i] - l[i]).abs().amax(dim=2) / (1 + l[i].abs().amax(dim=2)))[both].max()) for i in range(3))
        return {"vjp_many_against_ce_vjp": ev, "jvp_many_against_ce_jvp_psd": ej, "status_equal_to_ce_jvp_psd": bool(torch.equal(m[3], l[3]))}


def worker():
    benches = {}
    print("ready", flush=True)
    for line in sys.stdin:
        req = json.loads(line)
        if req["B"] not in benches:
            benches[req["B"]] = Bench(req["B"])
        ms, fl = benches[req["B"]].measure(req["what"], req["K"])
        print(json.dumps({"ms": ms, "flagged": fl}), flush=True)


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


ROUTES = (("reverse_loop", dict()), ("reverse_many", dict(solver_args={"psd_adjoint": "search_free"})),
          ("forward_loop", dict(direction="forward")), ("forward_many", dict(direction="forward", solver_args={"psd_tangents": "many"})))


def layer_jacobian(reps, B=1024):
    """CvxpyLayer.jacobian whole in both directions, with and without the keys, alternating; each includes the forward solve"""
    from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
    from cvxpylayers_amd.torch.templates import template_from_affine_builder
    m = P.cone_rows(CONES)
    A, b, c = P.generate(N, CONES, B, seed=SEED)
    tpl = template_from_affine_builder(lambda Ap, bp, cp: (Ap, bp, cp), [(m, N), (m,), (N,)], CONES, [VariableRecovery(slice(0, N), None, (N,))])
    layer = CvxpyLayer(template=tpl, solver_args={"eps": EPS, "max_iters": 100000, "raise_on_error": False})
    params = [torch.from_numpy(t).cuda() for t in (A, b, c)]
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    t, paths, flagged, err = {k: [] for k, _ in ROUTES}, {}, {}, {}
    for it in range(1 + reps):
        jac = {}
        for key, kw in ROUTES:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            _, j = layer.jacobian(*params, **kw)
            torch.cuda.synchronize(); ms = (time.perf_counter() - t0) * 1e3
            fwd = key.startswith("forward")
            paths[key] = [eng.last_jvp_many_path, layer.info["jvp"]["kernel"]] if fwd else [eng.last_vjp_many_path, layer.info["adjoint"]["path"]]
            st = layer.info["jvp"]["status"] if fwd else layer.info["adjoint"]["status"]
            flagged[key] = int((st != 0).any(dim=0).sum())
            jac[key] = (j, (st == 0).all(dim=0))
            if it >= 1:
                t[key].append(ms)
        want, ok = jac["reverse_loop"]
        for key in ("reverse_many", "forward_loop", "forward_many"):
            both = ok & jac[key][1]
            err[key + "_against_reverse_loop_on_unflagged"] = max(float(torch.nan_to_num(f[both] - r[both]).abs().max() / (1 + torch.nan_to_num(r[both]).abs().max()))
                                                                  for f, r in zip(jac[key][0][0], want[0]))
        del jac
    return {"B": B, "outputs": N, "parameter_entries": tpl.n_params_total, "reps": reps, "layer": "lqr_like with parameters A (36 x 24), b and c; x is the output",
            "wall_ms": {k: stat(v) for k, v in t.items()}, "paths": paths, "flagged_instances": flagged, **err}


def main():
    benches = {B: Bench(B) for B in sorted({B for B, _ in CASES})}
    child = None
    if a.parent:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--tree", os.path.abspath(a.parent)],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=os.path.abspath(a.parent))
        assert child.stdout.readline().strip() == "ready"
    plan = [("a_parent_ce_vjp", "vjp_sequential", True), ("b_ce_vjp", "vjp_sequential", False), ("c_ce_vjp_psd_many", "vjp_many", False),
            ("a_parent_ce_jvp_lsqr", "jvp_lsqr_sequential", True), ("a2_parent_ce_jvp_psd", "jvp_psd_sequential", True),
            ("b_ce_jvp_lsqr", "jvp_lsqr_sequential", False), ("b2_ce_jvp_psd", "jvp_psd_sequential", False), ("c_ce_jvp_psd_many", "jvp_many", False)]
    rows = []
    for B, K in CASES:
        bench = benches[B]
        t, fl = {k: [] for k, _, _ in plan}, {}
        for it in range(a.warmup + a.reps):
            for key, what, parent in plan:
                if parent:
                    if child is None:
                        continue
                    child.stdin.write(json.dumps({"B": B, "K": K, "what": what}) + "\n"); child.stdin.flush()
                    r = json.loads(child.stdout.readline())
                    ms, fl[key] = r["ms"], r["flagged"]
                else:
                    ms, fl[key] = bench.measure(what, K)
                if it >= a.warmup:
                    t[key].append(ms)
        st = {k: stat(v) for k, v in t.items() if v}
        row = {"B": B, "K": K, "wall_ms": st, "per_right_hand_side_ms": {k: v["median"] / K for k, v in st.items()}, "flagged": fl,
               "flagged_share": {k: v / B for k, v in fl.items()}, "unsolved_instances": bench.unsolved, "max_rel_difference_on_status_0": bench.agreement(K)}
        ref_v, ref_l = st.get("a_parent_ce_vjp", st["b_ce_vjp"]), st.get("a_parent_ce_jvp_lsqr", st["b_ce_jvp_lsqr"])
        ref_p = st.get("a2_parent_ce_jvp_psd", st["b2_ce_jvp_psd"])
        row["bracket_below"] = {"ce_vjp_psd_many_below_K_ce_vjp": st["c_ce_vjp_psd_many"]["max"] < ref_v["min"],
                                "ce_jvp_psd_many_below_K_ce_jvp_lsqr": st["c_ce_jvp_psd_many"]["max"] < ref_l["min"],
                                "ce_jvp_psd_many_below_K_ce_jvp_psd": st["c_ce_jvp_psd_many"]["max"] < ref_p["min"]}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    if child is not None:
        child.stdin.close(); child.wait(timeout=60)
    b0 = benches[CASES[0][0]]
    res = {"config": "lqr_like", "eps": EPS, "n": N, "m": b0.tpl.m, "nnz_aug": b0.tpl.nnz_aug, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "parent": bool(a.parent), "rows": rows}
    del benches
    if not a.no_layer:
        try:
            res["layer_jacobian"] = layer_jacobian(a.layer_reps)
        except Exception as e:          # (a record of the calls is worth keeping when the layer comparison fails)
            res["layer_jacobian"] = {"error": f"{type(e).__name__}: {e}"}
        print(json.dumps({"layer_jacobian": res["layer_jacobian"]}), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    worker() if a.worker else main()
