"""Time of solver_args param_grad="factors" on the QP / exponential / PSD many-cotangent kinds against the dA route under the same many-cotangent key, one box
(DESIGN.md section 3.22).  Wall time with the device idle before the clock starts and after it stops, the routes alternating per repetition; medians of --reps
after --warmup with min and max.  B = 1024, K = the layer's outputs (n).

  shapes: lqr_like (n = 24, PSD blocks 6 and 4), logdet_like (n = 20, a PSD block of 6 beside three exponential cones), E (the logistic-regression configuration,
          exponential cones), parameters (A, b, c); qp2 (the box QP of BASELINE configuration 2, n = 50, native) with parameters (b, q) and with P as a third;
  (a) CvxpyLayer.jacobian(direction="reverse") whole (the forward solve included) under the kind's many key, with and without param_grad="factors";
  (b) the engine calls at the point of one forward call: ConeEngine.vjp_many_params against vjp_many plus the transposed-map passes of the frontend.
With --parent TREE (a checkout of the parent commit with its library built) a child process serves the dA route of that build, one measurement at a time,
alternating with this build's.  Flagged instances are counted, not refused: both routes re-solve the same ones.

    python scripts/param_grad_kinds_timing.py [--reps 30] [--warmup 3] [--parent TREE] [--only NAME,...] [--out profiles/param_grad_kinds/kinds.json]
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
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--B", type=int, default=1024)
    ap.add_argument("--worker", action="store_true")          # (internal: serve single measurements of the tree in --tree over stdin / stdout)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    return ap.parse_args()


a = _args()
sys.path.insert(0, a.tree)

import torch  # noqa: E402

from cvxpylayers_amd import problems as P  # noqa: E402
from cvxpylayers_amd.interfaces import get_torch_cvxpylayer  # noqa: E402
from cvxpylayers_amd.torch import CvxpyLayer, VariableRecovery  # noqa: E402
from cvxpylayers_amd.torch.cvxpylayer import _spmm_bm  # noqa: E402
from cvxpylayers_amd.torch.templates import template_from_affine_builder  # noqa: E402

EPS = 1e-8
KEY = {"param_grad": "factors"}
CONES = {"lqr_like": (24, {"z": 3, "l": 2, "q": [], "s": [6, 4]}, 3, {"psd_adjoint": "search_free"}),
         "logdet_like": (20, {"z": 2, "l": 3, "q": [], "s": [6], "ep": 3}, 3, {"psd_adjoint": "search_free"}),
         "E": (P.CONFIGS["E"]["n"], P.CONFIGS["E"]["cones"], 3, {"tri_adjoint": "search_free"})}
QP_KEY = {"qp_adjoint": "search_free"}
NAMES = list(CONES) + ["qp2_bq", "qp2_bqP"]


def sync_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


class Case:
    def __init__(self, name, B):
        self.name, self.B, self.dev = name, B, torch.device("cuda", 0)
        args = {"eps": EPS, "max_iters": 100000}
        if name in CONES:
            n, cones, seed, self.many = CONES[name]
            m = P.cone_rows(cones)
            A, b, c = P.generate(n, cones, B, seed=seed)
            tpl = template_from_affine_builder(lambda Ap, bp, cp: (Ap, bp, cp), [(m, n), (m,), (n,)], cones, [VariableRecovery(slice(0, n), None, (n,))])
            ps = (A, b, c)
        else:          # the box QP of tests/qp_ns_kit.box_qp: min 1/2 x^T P x + q^T x, lo <= x <= hi
            n, self.many = 50, QP_KEY
            rng = np.random.default_rng(0)
            Fm = rng.standard_normal((n, n)) / np.sqrt(n); g = rng.standard_normal((B, n))
            lo = -0.5 - 0.5 * rng.random((B, n)); hi = 0.5 + 0.5 * rng.random((B, n))
            Pn = np.broadcast_to(2 * Fm.T @ Fm, (B, n, n)) * (1 + 0.1 * rng.random((B, 1, 1)))
            An = np.concatenate([-np.eye(n), np.eye(n)], axis=0)
            cones = {"z": 0, "l": 2 * n, "q": [], "s": []}
            P0 = 2 * Fm.T @ Fm
            rec = [VariableRecovery(slice(0, n), None, (n,))]
            if name == "qp2_bq":
                tpl = template_from_affine_builder(lambda bp, qp: (An, bp, qp, P0), [(2 * n,), (n,)], cones, rec)
                ps = (np.concatenate([-lo, hi], axis=1), -2 * g @ Fm)
            else:
                tpl = template_from_affine_builder(lambda bp, qp, Pp: (An, bp, qp, 0.5 * (Pp + Pp.T)), [(2 * n,), (n,), (n, n)], cones, rec)
                ps = (np.concatenate([-lo, hi], axis=1), -2 * g @ Fm, np.ascontiguousarray(Pn))
        self.n = n
        self.layer = CvxpyLayer(template=tpl, solver_args=args)
        self.params = [torch.from_numpy(np.ascontiguousarray(t)).to(self.dev) for t in ps]
        self._saved = None

    def jacobian(self, key):
        sa = {**self.many, **(KEY if key else {})}
        ms, _ = sync_ms(lambda: self.layer.jacobian(*self.params, solver_args=sa)[1][0][0].shape)
        adj = self.layer.info["adjoint"]
        return ms, int((adj["status"] != 0).sum()), {"path": adj.get("path"), "param_grad": adj.get("param_grad")}

    def saved(self):
        """the node of one forward call under the many key, as CvxpyLayer.jacobian obtains it: the engine, the point and the values the engine calls need"""
        if self._saved is None:
            layer, dev = self.layer, self.dev
            with torch.no_grad():
                p_bm = layer._flatten_params(self.params, layer.validate_params(list(self.params))).contiguous()
                A_eval, q_eval = _spmm_bm(layer._A.on(dev)[0], p_bm).t(), _spmm_bm(layer._q.on(dev)[0], p_bm).t()
                P_eval = _spmm_bm(layer._P.on(dev)[0], p_bm).t() if layer._P is not None else None
                _, _, _, data = get_torch_cvxpylayer(layer.solver).apply(P_eval, q_eval, A_eval, layer.ctx, self.many, True, None)
            g = torch.Generator(device="cpu").manual_seed(5)
            self._saved = (data[0], torch.randn((self.n, self.B, self.n), generator=g, dtype=torch.float64).to(dev))
        return self._saved

    def engine(self, key):
        sv, dx = self.saved()
        eng, layer, dev = sv.eng, self.layer, self.dev
        K, B = dx.shape[:2]
        flags = dict(qp_many="qp_adjoint" in self.many, tri_many="tri_adjoint" in self.many, psd_many="psd_adjoint" in self.many)
        if key:
            maps = layer._pg_maps()
            ms, out = sync_ms(lambda: eng.vjp_many_params(sv.A_bm, sv.x, sv.y, sv.s, dx, None, maps, lsqr=sv.lsqr, q_eval=sv.q_eval, P_bm=sv.P_bm, **flags))
            return ms, int((out[2] != 0).sum()), {"kernel": eng.last_vjp_kernel}
        bA, bq = layer._A.on(dev)[1], layer._q.on(dev)[1]
        def run():
            out = eng.vjp_many(sv.A_bm, sv.x, sv.y, sv.s, dx, None, path=sv.path, lsqr=sv.lsqr, q_eval=sv.q_eval, P_bm=sv.P_bm, **flags)
            g = torch.empty((K * B, bA[3]), dtype=torch.float64, device=dev)
            _spmm_bm(bA, out[0].view(K * B, -1), out=g.zero_())
            _spmm_bm(bq, out[1].view(K * B, -1), out=g)
            if sv.P_bm is not None:
                _spmm_bm(layer._P.on(dev)[1], out[3].contiguous().view(K * B, -1), out=g)
            return out[2]
        ms, adj = sync_ms(run)
        return ms, int((adj != 0).sum()), {"kernel": eng.last_vjp_kernel}

    def measure(self, what, key):
        return (self.jacobian if what == "jacobian" else self.engine)(key)


_CASES: dict = {}


def case(name, B):
    if name not in _CASES:
        _CASES[name] = Case(name, B)
    return _CASES[name]


def worker():
    print("ready", flush=True)
    for line in sys.stdin:
        req = json.loads(line)
        ms, fl, _ = case(req["name"], req["B"]).measure(req["what"], False)
        print(json.dumps({"ms": ms, "flagged": fl}), flush=True)


def stat(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def main():
    child = None
    if a.parent:
        child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--worker", "--tree", os.path.abspath(a.parent)],
                                 stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, cwd=os.path.abspath(a.parent))
        assert child.stdout.readline().strip() == "ready"
    rows = []
    for name in (a.only.split(",") if a.only else NAMES):
        for what in ("jacobian", "engine"):
            t = {"parent_dA": [], "dA": [], "factors": []}
            flagged, route = {}, {}
            for it in range(a.warmup + a.reps):
                if child is not None:
                    child.stdin.write(json.dumps({"name": name, "B": a.B, "what": what}) + "\n"); child.stdin.flush()
                    r = json.loads(child.stdout.readline())
                    if it >= a.warmup:
                        t["parent_dA"].append(r["ms"])
                for r_, key in (("dA", False), ("factors", True)):
                    ms, fl, info = case(name, a.B).measure(what, key)
                    flagged[r_], route[r_] = fl, info
                    if it >= a.warmup:
                        t[r_].append(ms)
            row = {"name": name, "what": what, "B": a.B, "K": case(name, a.B).n, "reps": a.reps, "wall_ms": {k: stat(v) for k, v in t.items() if v},
                   "flagged_pairs": flagged, "route": route}
            row["factors_over_dA"] = row["wall_ms"]["factors"]["median"] / row["wall_ms"]["dA"]["median"]
            rows.append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    if child is not None:
        child.stdin.close(); child.wait(timeout=60)
    res = {"eps": EPS, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "parent": bool(a.parent), "rows": rows}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    worker() if a.worker else main()
