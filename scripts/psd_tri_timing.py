"""Times of the search-free elimination on a template with PSD blocks AND exponential / power triples (ce_jvp_psd_tri, ce_refine_psd_tri, ce_vjp_psd_tri_many,
ce_jvp_psd_tri_many) against the routes such a template has without them, one box.

Shape logdet_like (tests/psd_tri_ns_kit.py: n = 20, 2 zero and 3 nonnegative rows, one PSD block of order 6, three exponential cones, m = 35) at the eps = 1e-8
point.  Per case wall time with the device idle before the clock starts and after it stops, the routes interleaved per repetition:
  single     ce_jvp_psd_tri against ce_jvp_lsqr (with its mean iteration count) and against the pivoting ce_vjp, B = 4096; one ce_refine_psd_tri step;
  refine     the solve at eps = 1e-4 plus two ce_refine_psd_tri steps against the solve at eps = 1e-8, with the distance of the first 64 instances to the CPU
             oracle's eps = 1e-10 point;
  many       ce_vjp_psd_tri_many against K pivoting ce_vjp calls, ce_jvp_psd_tri_many against K ce_jvp_lsqr and K ce_jvp_psd_tri calls, at (B = 4096, K = 8),
             (B = 4096, K = 1) and (B = 1024, K = n);
  layer      CvxpyLayer.jacobian whole at B = 1024 in both directions for a layer on that shape with parameters A, b and c and output x, with and without the keys.
The comparator routes (ce_vjp, ce_jvp_lsqr, the solve) are also run by ANOTHER BUILD of this repository (--parent TREE: a checkout of the parent commit with its
library built) in a child process that is asked for one measurement at a time, alternating with this build's -- omitted without --parent.  All under the default
re-solve rule with q_eval given; outputs are allocated inside the clock.  Medians of --reps after --warmup calls, with min and max, and the share of flagged
instances.  Prints one JSON line; --out also writes it.

    python scripts/psd_tri_timing.py [--reps 30] [--warmup 5] [--parent TREE] [--out profiles/psd_tri/psd_tri_logdet_like.json]
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
N, CONES = 20, {"z": 2, "l": 3, "s": [6], "ep": 3}          # tests/psd_tri_ns_kit.py SHAPES["logdet_like"]
CASES = ((4096, 8), (4096, 1), (1024, N))          # (B, K)


class Bench:
    """logdet_like at batch size B, solved by the build that runs this at eps 1e-8, and Gaussian right-hand sides"""

    def __init__(self, B):
        self.B = B
        self.dev = torch.device("cuda", 0)
        self.data = P.generate(N, CONES, B, seed=SEED)
        self.tpl = P.dense_template(N, CONES)
        self.eng = ConeEngine(self.tpl.indices, self.tpl.indptr, self.tpl.n, self.tpl.m, self.tpl.cones, self.dev)
        A_eval, q_eval = self.tpl.values_from_dense(*self.data)
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
        assert self.eng.last_vjp_kernel == "ce_vjp_psd_tri_many"
        return r

    def jvp_sequential(self, K, psd_ns):
        _, _, tA, tq = self.rhs(K)
        kw = {"psd_ns": True} if psd_ns else {}          # (the parent's jvp is never asked for the flag)
        r = self._timed(lambda: [self.eng.jvp(self.A_bm, *self.pt, tA[k], tq[k].t(), path="per_instance", q_eval=self.q_t, method="direct", **kw) for k in range(K)][0][3])
        assert self.eng.last_jvp_kernel == ("ce_jvp_psd_tri" if psd_ns else "ce_jvp_lsqr")
        self.last_iters = float(self.eng.last_lsqr_iters.double().mean())
        return r

    def jvp_many(self, K):
        _, _, tA, tq = self.rhs(K)
        r = self._timed(lambda: self.eng.jvp_many(self.A_bm, *self.pt, tA, tq, path="per_instance", q_eval=self.q_t, method="direct", psd_many=True)[3][0])
        assert self.eng.last_jvp_kernel == "ce_jvp_psd_tri_many"
        return r

    def refine_step(self, K):
        def run():
            x, y, s = (t.clone() for t in self.pt)
            info = self.eng.refine(self.A_bm, self.q_t, x, y, s, 1, psd_ns=True)[3]
            assert info["path"] == "ns"
            return (info["status"] & 4)
        return self._timed(run)

    def solve(self, eps, steps):
        def run():
            out = self.eng.solve(self.A_bm, self.q_t, make_settings({"eps": eps, "max_iters": 100000}))
            x, y, s = out[:3]
            if steps:
                x, y, s, info = self.eng.refine(self.A_bm, self.q_t, x, y, s, steps, status=out[4], psd_ns=True)
                assert info["path"] == "ns"
            self.last_point = (x, y, s)
            return (out[4] != 1).to(torch.int32)
        return self._timed(run)

    def measure(self, what, K):
        return {"vjp_sequential": lambda: self.vjp_sequential(K), "vjp_many": lambda: self.vjp_many(K), "jvp_lsqr_sequential": lambda: self.jvp_sequential(K, False),
                "jvp_psd_tri_sequential": lambda: self.jvp_sequential(K, True), "jvp_many": lambda: self.jvp_many(K), "refine_step": lambda: self.refine_step(K),
                "solve_1e-8": lambda: self.solve(1e-8, 0), "solve_1e-4_two_steps": lambda: self.solve(1e-4, 2)}[what]()

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
        return {"vjp_many_against_ce_vjp": ev, "jvp_many_against_ce_jvp_psd_tri": ej, "status_equal_to_ce_jvp_psd_tri": bool(torch.equal(m[3], l[3]))}


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
    return {"B": B, "outputs": N, "parameter_entries": tpl.n_params_total, "reps": reps, "layer": f"logdet_like with parameters A ({m} x {N}), b and c; x is the output",
            "wall_ms": {k: stat(v) for k, v in t.items()}, "paths": paths, "flagged_instances": flagged, **err}


def oracle_distance(bench, n_sample=64):
    """max-norm distance of the first n_sample instances' (x, y, s) to the CPU oracle's eps = 1e-10 point, for the two solve routes"""
    sys.path.insert(0, a.tree)
    from oracle import oracle
    A, b, c = (t[:n_sample] for t in bench.data)
    hi = oracle.solve_batch(A, b, c, CONES, eps=1e-10, max_iters=200000)
    out = {}
    for what in ("solve_1e-8", "solve_1e-4_two_steps"):
        bench.measure(what, 1)
        d = np.max([np.abs(t[:n_sample].cpu().numpy() - hi[k]).max(axis=1) for t, k in zip(bench.last_point, "xys")], axis=0)[hi["status"] == 1]
        out[what] = {"median": float(np.median(d)), "max": float(d.max()), "instances": int(d.size)}
    return out


def main():
    benches = {B: Bench(B) for B in sorted({B for B, _ in CASES})}
    child = None
    if a.parent:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--tree", os.path.abspath(a.parent)],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=os.path.abspath(a.parent))
        assert child.stdout.readline().strip() == "ready"

    def run(plan, B, K):
        bench = benches[B]
        t, fl, extra = {k: [] for k, _, _ in plan}, {}, {}
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
                    if what == "jvp_lsqr_sequential":
                        extra["ce_jvp_lsqr_mean_iterations"] = bench.last_iters
                if it >= a.warmup:
                    t[key].append(ms)
        return {k: stat(v) for k, v in t.items() if v}, fl, extra

    # ---- one right-hand side, one refinement step, and the two solve routes, B = 4096
    single_plan = [("a_parent_ce_jvp_lsqr", "jvp_lsqr_sequential", True), ("a_parent_ce_vjp", "vjp_sequential", True), ("b_ce_jvp_lsqr", "jvp_lsqr_sequential", False),
                   ("b_ce_vjp", "vjp_sequential", False), ("c_ce_jvp_psd_tri", "jvp_psd_tri_sequential", False), ("c_one_ce_refine_psd_tri_step", "refine_step", False)]
    st, fl, extra = run(single_plan, 4096, 1)
    single = {"B": 4096, "wall_ms": st, "flagged": fl, "flagged_share": {k: v / 4096 for k, v in fl.items()}, **extra}
    print(json.dumps({"single": single}), file=sys.stderr, flush=True)
    solve_plan = [("a_parent_solve_1e-8", "solve_1e-8", True), ("b_solve_1e-8", "solve_1e-8", False), ("c_solve_1e-4_two_steps", "solve_1e-4_two_steps", False)]
    st, fl, _ = run(solve_plan, 4096, 1)
    refine = {"B": 4096, "wall_ms": st, "unsolved": fl, "distance_to_the_oracle_point_first_64": oracle_distance(benches[4096])}
    print(json.dumps({"refine": refine}), file=sys.stderr, flush=True)
    # ---- K right-hand sides
    plan = [("a_parent_ce_vjp", "vjp_sequential", True), ("b_ce_vjp", "vjp_sequential", False), ("c_ce_vjp_psd_tri_many", "vjp_many", False),
            ("a_parent_ce_jvp_lsqr", "jvp_lsqr_sequential", True), ("b_ce_jvp_lsqr", "jvp_lsqr_sequential", False), ("b2_ce_jvp_psd_tri", "jvp_psd_tri_sequential", False),
            ("c_ce_jvp_psd_tri_many", "jvp_many", False)]
    rows = []
    for B, K in CASES:
        st, fl, extra = run(plan, B, K)
        row = {"B": B, "K": K, "wall_ms": st, "per_right_hand_side_ms": {k: v["median"] / K for k, v in st.items()}, "flagged": fl,
               "flagged_share": {k: v / B for k, v in fl.items()}, "unsolved_instances": benches[B].unsolved, "max_rel_difference_on_status_0": benches[B].agreement(K), **extra}
        ref_v, ref_l = st.get("a_parent_ce_vjp", st["b_ce_vjp"]), st.get("a_parent_ce_jvp_lsqr", st["b_ce_jvp_lsqr"])
        row["bracket_below"] = {"ce_vjp_psd_tri_many_below_K_ce_vjp": st["c_ce_vjp_psd_tri_many"]["max"] < ref_v["min"],
                                "ce_jvp_psd_tri_many_below_K_ce_jvp_lsqr": st["c_ce_jvp_psd_tri_many"]["max"] < ref_l["min"],
                                "ce_jvp_psd_tri_many_below_K_ce_jvp_psd_tri": st["c_ce_jvp_psd_tri_many"]["max"] < st["b2_ce_jvp_psd_tri"]["min"]}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    if child is not None:
        child.stdin.close(); child.wait(timeout=60)
    b0 = benches[CASES[0][0]]
    res = {"config": "logdet_like", "eps": EPS, "n": N, "m": b0.tpl.m, "nnz_aug": b0.tpl.nnz_aug, "reps": a.reps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0), "parent": bool(a.parent), "single": single, "refine": refine, "rows": rows}
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
