"""Cost and effect of solver_args newton_first at the metric configuration, one process per build, one box.

The previous point is the engine's own solve of the unperturbed batch at the call's eps; the call's data is that batch with every entry of A, b, c multiplied by
1 + rel N(0, 1) (default_rng(seed + 100), in that order).  For rel in {1e-3, 1e-2, 1e-1} x eps in {1e-4, 1e-8}, wall time of one plugin forward
(_CvxpyLayer.apply, needs_grad=False, explicit warm triple; the device is idle before the clock starts and after it stops), alternating per repetition:
  (a) the warm-started forward of ANOTHER BUILD of this repository (--parent TREE: a checkout of the parent commit with its library built), run by a child
      process that is asked for one call at a time -- omitted without --parent;
  (b) this build, newton_first = 0;
  (c) this build, newton_first = k for k in {1, 2, 3}, with n_fallback.
Then, for every (c), the pieces by hand with events on the stream: the refine launches, ce_check_solved, the 4-byte host read (wall), gather + sub-batch solve +
scatter.  Last, ce_check_solved alone next to ce_transpose of the same array and one ce_refine step, with its rate over its algorithmic bytes
8 (nnz_aug + 2 n + 1 + 3 m) per instance.  Medians of --reps after --warmup calls, with min and max.  A configuration in which an instance fails (the 10 %
change makes some infeasible) is timed under raise_on_error=False in all variants, and says so.  Prints one JSON line; --out also writes it.

    python scripts/newton_first_timing.py [--B 4096] [--reps 30] [--warmup 5] [--parent TREE] [--check-only] [--out profiles/newton_first/newton_first_M.json]
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
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--check-only", action="store_true", help="time ce_check_solved beside ce_transpose and one ce_refine step, nothing else")
    ap.add_argument("--worker", action="store_true")          # (internal: serve single calls of the tree in --tree over stdin / stdout)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    return ap.parse_args()


a = _args()
sys.path.insert(0, a.tree)

import torch  # noqa: E402

from cvxpylayers_amd import problems as P  # noqa: E402
from cvxpylayers_amd.interfaces.mi355_if import MI355_ctx, SolverError, _CvxpyLayer, make_settings  # noqa: E402

SEED = 11
RELS, EPSS, KS = (1e-3, 1e-2, 1e-1), (1e-4, 1e-8), (1, 2, 3)


class Bench:
    """the metric batch, its perturbed copies and the previous points of one build"""

    def __init__(self, B):
        cfg = P.CONFIGS["M"]
        self.n, self.cones, self.B = cfg["n"], cfg["cones"], B
        self.tpl = P.dense_template(self.n, self.cones)
        self.base = P.generate(self.n, self.cones, B, seed=SEED)
        self.ctx = MI355_ctx(None, self.tpl.problem_data_index, self.cones)
        self.dev = torch.device("cuda", 0)
        self.eng = self.ctx.engine(self.dev)
        self._data, self._warm = {}, {}

    def tensors(self, A, b, c):
        A_eval, q_eval = self.tpl.values_from_dense(A, b, c)
        return torch.from_numpy(np.ascontiguousarray(A_eval.T)).to(self.dev).t(), torch.from_numpy(q_eval).to(self.dev)          # (batch-major values: no layout pass in the call)

    def data(self, rel):
        if rel not in self._data:
            rng = np.random.default_rng(SEED + 100)
            self._data[rel] = self.tensors(*(t * (1.0 + rel * rng.standard_normal(t.shape)) for t in self.base))
        return self._data[rel]

    def warm(self, eps):
        if eps not in self._warm:
            A_t, q_t = self.tensors(*self.base)
            _CvxpyLayer.apply(None, q_t, A_t, self.ctx, {"eps": eps}, False, None)
            self._warm[eps] = tuple(t.clone() for t in self.eng._last_solution)
        return self._warm[eps]

    def call(self, rel, eps, k, roe=True):
        """one forward: (wall ms, info)"""
        A_t, q_t = self.data(rel)
        w = self.warm(eps)
        args = {"eps": eps}
        if k:
            args["newton_first"] = k
        if not roe:
            args["raise_on_error"] = False
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, info, _ = _CvxpyLayer.apply(None, q_t, A_t, self.ctx, args, False, w)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, info


def worker():
    bench = Bench(a.B)
    print("ready", flush=True)
    for line in sys.stdin:
        req = json.loads(line)
        ms, info = bench.call(req["rel"], req["eps"], 0, req["roe"])
        print(json.dumps({"ms": ms, "iters_mean": float(info["iters"].double().mean())}), flush=True)


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def ev_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record(); e1.synchronize()
    return e0.elapsed_time(e1), out


def pieces(bench, rel, eps, k):
    """the flow of interfaces/newton_first.py by hand, one piece per event pair"""
    from cvxpylayers_amd.interfaces.newton_first import _read_int
    eng = bench.eng
    A_t, q_t = bench.data(rel)
    A_bm = A_t.t()
    st = make_settings({"eps": eps})
    out = {"refine": [], "check": [], "host_read_wall": [], "fallback": []}
    for it in range(a.warmup + a.reps):
        x, y, s = (t.clone() for t in bench.warm(eps))
        torch.cuda.synchronize()
        t_ref, (x, y, s, ri) = ev_ms(lambda: eng.refine(A_bm, q_t, x, y, s, k))
        t_chk, (solved, status, iters, resid, n_uns) = ev_ms(lambda: eng.check_solved(A_t, q_t, x, y, s, st.eps_abs, st.eps_rel, eligible=ri["status"]))
        t0 = time.perf_counter(); nfb = _read_int(eng, n_uns); t_read = (time.perf_counter() - t0) * 1e3

        def fallback():
            if nfb == 0:
                return
            idx = torch.argsort(solved.to(torch.int32), stable=True)[:nfb]
            sub = eng.solve_transient(A_bm.index_select(0, idx), q_t.index_select(1, idx), st, warm=(x.index_select(0, idx), y.index_select(0, idx), s.index_select(0, idx)), path="per_instance")
            for full, part in zip((x, y, s, iters, status, resid), sub):
                full.index_copy_(0, idx, part)
        t_fb, _ = ev_ms(fallback)
        if it >= a.warmup:
            out["refine"].append(t_ref); out["check"].append(t_chk); out["host_read_wall"].append(t_read); out["fallback"].append(t_fb)
    return {k_: stat(v) for k_, v in out.items()}


def check_alone(bench):
    eng, n, m, K, B = bench.eng, bench.n, bench.tpl.m, bench.tpl.nnz_aug, bench.B
    A_t, q_t = bench.data(1e-3)
    A_bm = A_t.t()
    A_minor = A_t.contiguous()          # (nnz_aug, B) contiguous: what ce_transpose turns into batch-major rows
    w = bench.warm(1e-8)
    times = {"ce_check_solved": [], "ce_transpose": [], "ce_refine_1_step": []}
    for it in range(a.warmup + a.reps):
        x, y, s = (t.clone() for t in w)
        torch.cuda.synchronize()
        for name, fn in (("ce_check_solved", lambda: eng.check_solved(A_t, q_t, x, y, s, 1e-8, 1e-8)), ("ce_transpose", lambda: eng.to_batch_major(A_minor)),
                         ("ce_refine_1_step", lambda: eng.refine(A_bm, q_t, x, y, s, 1))):
            t, _ = ev_ms(fn)
            if it >= a.warmup:
                times[name].append(t)
    res = {k_: stat(v) for k_, v in times.items()}
    # the same three by the library's own event brackets (no Python between the events): mean ms per call
    x, y, s = (t.clone() for t in w)
    for name, which, fn in (("ce_check_solved", 2, lambda: eng.check_solved(A_t, q_t, x, y, s, 1e-8, 1e-8)), ("ce_transpose", 2, lambda: eng.to_batch_major(A_minor)),
                            ("ce_refine_1_step", 1, lambda: eng.refine(A_bm, q_t, x, y, s, 1))):
        eng.set_profiling(True); eng.reset_profile()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        res[name]["bracket_mean"] = eng.profile(which)[0]
        eng.set_profiling(0); eng.reset_profile()
    nbytes = 8.0 * (K + 2 * n + 1 + 3 * m) * B
    res["check_bytes"] = nbytes
    res["check_GB_per_s"] = nbytes / (res["ce_check_solved"]["bracket_mean"] * 1e-3) / 1e9
    res["note"] = "median / min / max: events around the Python call (its allocations and fills included); bracket_mean: the library's events around the launches alone (ce_check_solved: the test and the count), which the rate is taken over"
    return res


def main():
    bench = Bench(a.B)
    child = None
    if a.parent:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--tree", os.path.abspath(a.parent), "--B", str(a.B)],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=os.path.abspath(a.parent))
        assert child.stdout.readline().strip() == "ready"

    def ask(rel, eps, roe):
        child.stdin.write(json.dumps({"rel": rel, "eps": eps, "roe": roe}) + "\n"); child.stdin.flush()
        return json.loads(child.stdout.readline())

    rows = []
    for rel in (() if a.check_only else RELS):
        for eps in EPSS:
            roe = True
            try:
                bench.call(rel, eps, 0)
            except SolverError:
                roe = False
            t = {"a_parent": [], "b_k0": [], **{f"c_k{k}": [] for k in KS}}
            nfb, iters = {}, {}
            for it in range(a.warmup + a.reps):
                if child is not None:
                    r = ask(rel, eps, roe)
                    iters["a_parent"] = r["iters_mean"]
                    if it >= a.warmup:
                        t["a_parent"].append(r["ms"])
                for k in (0,) + KS:
                    ms, info = bench.call(rel, eps, k, roe)
                    key = f"c_k{k}" if k else "b_k0"
                    if it >= a.warmup:
                        t[key].append(ms)
                    iters[key] = float(info["iters"].double().mean())
                    if k:
                        nfb[key] = int(info["newton_first"]["n_fallback"])
            row = {"rel": rel, "eps": eps, "raise_on_error": roe, "forward_wall_ms": {k_: stat(v) for k_, v in t.items() if v}, "n_fallback": nfb, "iters_mean": iters,
                   "pieces_ms": {f"k{k}": pieces(bench, rel, eps, k) for k in KS}}
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    if child is not None:
        child.stdin.close(); child.wait(timeout=60)
    res = {"config": "M", "B": a.B, "n": bench.n, "m": bench.tpl.m, "nnz_aug": bench.tpl.nnz_aug, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "parent": bool(a.parent), "rows": rows, "check_alone_ms": check_alone(bench)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    worker() if a.worker else main()
