"""Time of K tangents at one solution of a template with exponential cones: ce_jvp_tri_many (the search-free elimination with triples, one factorisation per
instance, one LSQR launch for the flagged instances of every tangent; ConeEngine.jvp_many(tri_many=True)) against K sequential ce_jvp calls (the same elimination,
every triple diagonalised and every instance factored once per tangent, one LSQR walk per tangent), one box.

The logistic-regression shape E (problems.CONFIGS["E"]: n = 40, 12 nonnegative rows, one second-order block of 4, 24 exponential cones) at the eps = 1e-8 point:
B = 4096 with K = 1, 2, 8, and B = 1024 with K = n = 40; then CvxpyLayer.jacobian(direction="forward") whole at B = 1024 for a layer on shape E with parameters
A, b and c under both values of solver_args tri_tangents.

Per case wall time with the device idle before the clock starts and after it stops, alternating per repetition:
  (a) K sequential ConeEngine.jvp(method="direct") calls of ANOTHER BUILD of this repository (--parent TREE: a checkout of the parent commit with its library
      built), run by a child process that is asked for one measurement at a time -- omitted without --parent;
  (b) the same K sequential calls of this build;
  (c) this build's jvp_many(tri_many=True).
All three under the default re-solve rule with q_eval given; outputs are allocated inside the clock.  Medians of --reps after --warmup calls, with min and max, the
number of flagged instances and their mean LSQR iterations; per case also (b) and (c) on the sub-batch of the instances the stiff rule does not flag
(`without_flagged_instances`: the eliminations alone, an empty list behind them).  `resolve_ms_by_difference`: the median of (c) on the full batch minus the median
of (c) on the unflagged sub-batch scaled to the full batch size -- what the one re-solve launch costs, by difference (no clock sits between the two launches of a
call).  Prints one JSON line; --out also writes it.

    python scripts/jvp_tri_many_timing.py [--reps 30] [--warmup 5] [--parent TREE] [--out profiles/jvp_tri_many/jvp_tri_many_E.json]
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

SEED, EPS = 11, 1e-8
N = P.CONFIGS["E"]["n"]
CASES = ((4096, 1), (4096, 2), (4096, 8), (1024, N))          # (B, K)


class Bench:
    """shape E at batch size B, solved by this build at eps 1e-8, and Gaussian tangents"""

    def __init__(self, B):
        self.B = B
        self.dev = torch.device("cuda", 0)
        self.n, self.cones = N, P.CONFIGS["E"]["cones"]
        A, b, c = P.generate(self.n, self.cones, B, seed=SEED)
        self.tpl = P.dense_template(self.n, self.cones)
        self.eng = ConeEngine(self.tpl.indices, self.tpl.indptr, self.tpl.n, self.tpl.m, self.tpl.cones, self.dev)
        A_eval, q_eval = self.tpl.values_from_dense(A, b, c)
        self.A_bm = torch.from_numpy(np.ascontiguousarray(A_eval.T)).to(self.dev); self.q_t = torch.from_numpy(q_eval).to(self.dev)
        out = self.eng.solve(self.A_bm, self.q_t, make_settings({"eps": EPS, "max_iters": 100000}))
        self.pt = tuple(out[:3])
        self.unsolved = int((out[4] != 1).sum())
        self._cot = {}

    def tangents(self, K):
        """tA (K, B, nnz_aug), tq (K, B, n + 1), drawn on the device"""
        if K not in self._cot:
            g = torch.Generator(device=self.dev).manual_seed(SEED + K)
            self._cot = {K: tuple(torch.randn((K, self.B, w), generator=g, dtype=torch.float64, device=self.dev) for w in (self.tpl.nnz_aug, self.n + 1))}          # (one K at a time: the rows of tA are large)
        return self._cot[K]

    def sequential(self, K):
        """K ce_jvp calls: (wall ms, flagged instances, mean LSQR iterations of the flagged)"""
        tA, tq = self.tangents(K)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        outs = [self.eng.jvp(self.A_bm, *self.pt, tA[k], tq[k].t(), path="per_instance", q_eval=self.q_t, method="direct") for k in range(K)]
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        assert self.eng.last_jvp_kernel == "ce_jvp"
        fl = outs[0][3] != 0
        return ms, int(fl.sum()), float(self.eng.last_lsqr_iters[fl].double().mean()) if fl.any() else 0.0

    def many(self, K):
        tA, tq = self.tangents(K)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = self.eng.jvp_many(self.A_bm, *self.pt, tA, tq, path="per_instance", q_eval=self.q_t, method="direct", tri_many=True)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        assert self.eng.last_jvp_many_path == "many" and self.eng.last_jvp_kernel == "ce_jvp_tri_many"
        fl = out[3][0] != 0
        return ms, int(fl.sum()), float(self.eng.last_lsqr_iters[:, fl].double().mean()) if fl.any() else 0.0

    def without_flagged(self):
        """the same point restricted to the instances the stiff rule does not flag: an empty list behind either route there, the eliminations alone"""
        tA, tq = self.tangents(1)
        st = self.eng.jvp_many(self.A_bm, *self.pt, tA, tq, path="per_instance", q_eval=self.q_t, method="direct", tri_many=True)[3][0]
        keep = torch.nonzero(st == 0).flatten()
        sub = object.__new__(Bench)
        sub.__dict__.update(self.__dict__)
        sub.B, sub.A_bm, sub.q_t, sub.pt, sub._cot = int(keep.numel()), self.A_bm[keep].contiguous(), self.q_t[:, keep].contiguous(), tuple(t[keep].contiguous() for t in self.pt), {}
        return sub

    def agreement(self, K):
        """largest relative difference between the two routes on status-0 instances, and whether status, iterations and the flagged instances' values are equal"""
        tA, tq = self.tangents(K)
        kw = dict(path="per_instance", q_eval=self.q_t, method="direct")
        m = self.eng.jvp_many(self.A_bm, *self.pt, tA, tq, tri_many=True, **kw); im = self.eng.last_lsqr_iters
        l = self.eng.jvp_many(self.A_bm, *self.pt, tA, tq, force_loop=True, **kw); il = self.eng.last_lsqr_iters
        reg = m[3] == 0
        e = max(float(((m[i] - l[i]).abs().amax(dim=2) / (1 + l[i].abs().amax(dim=2)))[reg].max()) for i in range(3))
        same = bool(torch.equal(m[3], l[3]) and torch.equal(im, il) and all(torch.equal(m[i][~reg], l[i][~reg]) for i in range(3)))
        return e, same


def worker():
    benches = {}
    print("ready", flush=True)
    for line in sys.stdin:
        req = json.loads(line)
        if req["B"] not in benches:
            benches[req["B"]] = Bench(req["B"])
        ms, fl, its = benches[req["B"]].sequential(req["K"])
        print(json.dumps({"ms": ms, "flagged": fl, "iters": its}), flush=True)


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


ROUTES = (("forward_many", dict(direction="forward", solver_args={"tri_tangents": "many"})), ("forward_loop", dict(direction="forward")))


def layer_jacobian(reps, B=1024):
    """CvxpyLayer.jacobian(direction="forward") whole under both values of tri_tangents, alternating; each includes the forward solve"""
    from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery
    from cvxpylayers_amd.torch.templates import template_from_affine_builder
    cones = P.CONFIGS["E"]["cones"]
    m = P.cone_rows(cones)
    A, b, c = P.generate(N, cones, B, seed=SEED)
    tpl = template_from_affine_builder(lambda Ap, bp, cp: (Ap, bp, cp), [(m, N), (m,), (N,)], cones, [VariableRecovery(slice(0, N), None, (N,))])
    layer = CvxpyLayer(template=tpl, solver_args={"eps": EPS, "max_iters": 100000, "raise_on_error": False})
    params = [torch.from_numpy(t).cuda() for t in (A, b, c)]
    eng = layer.ctx.solver_ctx.engine(torch.device("cuda", 0))
    t, paths, flagged, err = {k: [] for k, _ in ROUTES}, {}, {}, {}
    for it in range(1 + reps):
        jac = {}
        for key, kw in ROUTES:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            _, jac[key] = layer.jacobian(*params, **kw)
            torch.cuda.synchronize(); ms = (time.perf_counter() - t0) * 1e3
            paths[key] = [eng.last_jvp_many_path, layer.info["jvp"]["kernel"]]
            st = layer.info["jvp"]["status"]
            flagged[key] = int((st[0] != 0).sum())
            jac[key] = (jac[key], st)
            if it >= 1:
                t[key].append(ms)
        both = ((jac["forward_many"][1] == 0) & (jac["forward_loop"][1] == 0)).all(dim=0)
        err["many_against_loop_on_unflagged"] = max(float(torch.nan_to_num(f[both] - r[both]).abs().max() / (1 + torch.nan_to_num(r[both]).abs().max()))
                                                    for f, r in zip(jac["forward_many"][0][0], jac["forward_loop"][0][0]))
        err["unflagged_by_both"] = int(both.sum())
        del jac
    return {"B": B, "outputs": N, "parameter_entries": tpl.n_params_total, "reps": reps, "layer": "shape E with parameters A (88 x 40), b and c; x is the output",
            "wall_ms": {k: stat(v) for k, v in t.items()}, "paths": paths, "flagged": flagged, **err}


def main():
    benches = {B: Bench(B) for B in sorted({B for B, _ in CASES})}
    child = None
    if a.parent:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--tree", os.path.abspath(a.parent)],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=os.path.abspath(a.parent))
        assert child.stdout.readline().strip() == "ready"
    rows, subs = [], {}
    for B, K in CASES:
        bench = benches[B]
        t = {"a_parent_sequential": [], "b_sequential": [], "c_many": []}
        fl, its = {}, {}
        for it in range(a.warmup + a.reps):
            if child is not None:
                child.stdin.write(json.dumps({"B": B, "K": K}) + "\n"); child.stdin.flush()
                r = json.loads(child.stdout.readline())
                fl["a_parent_sequential"], its["a_parent_sequential"] = r["flagged"], r["iters"]
                if it >= a.warmup:
                    t["a_parent_sequential"].append(r["ms"])
            for key, fn in (("b_sequential", bench.sequential), ("c_many", bench.many)):
                ms, fl[key], its[key] = fn(K)
                if it >= a.warmup:
                    t[key].append(ms)
        st = {k_: stat(v) for k_, v in t.items() if v}
        row = {"B": B, "K": K, "wall_ms": st, "per_tangent_ms": {k_: v["median"] / K for k_, v in st.items()}, "flagged": fl,
               "flagged_share": {k_: v / B for k_, v in fl.items()}, "mean_lsqr_iterations_of_flagged": its, "unsolved_instances": bench.unsolved}
        row["max_rel_difference_on_status_0"], row["status_iterations_and_flagged_values_equal_to_the_loop"] = bench.agreement(K)
        sub = subs.setdefault(B, bench.without_flagged())          # (the flagged instances left out: what the eliminations cost with an empty list behind them)
        ts = {"b_sequential": [], "c_many": []}
        fls = {}
        for it in range(a.warmup + a.reps):
            for key, fn in (("b_sequential", sub.sequential), ("c_many", sub.many)):
                ms, fls[key], _ = fn(K)
                if it >= a.warmup:
                    ts[key].append(ms)
        row["without_flagged_instances"] = {"B": sub.B, "wall_ms": {k_: stat(v) for k_, v in ts.items()}, "flagged": fls}
        row["resolve_ms_by_difference"] = st["c_many"]["median"] - row["without_flagged_instances"]["wall_ms"]["c_many"]["median"] * B / sub.B
        ref = st.get("a_parent_sequential", st["b_sequential"])
        row["many_bracket_below_sequential"] = st["c_many"]["max"] < ref["min"]
        rows.append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    if child is not None:
        child.stdin.close(); child.wait(timeout=60)
    b0 = benches[CASES[0][0]]
    res = {"config": "E", "eps": EPS, "n": b0.n, "m": b0.tpl.m, "nnz_aug": b0.tpl.nnz_aug, "reps": a.reps, "warmup": a.warmup,
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
