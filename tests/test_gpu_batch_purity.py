"""An instance's result depends only on its own inputs.  On one representative shape per distinct forward plan and per distinct adjoint plan found by
tests/test_gpu_plan_edges.py's discovery, the answer of a fresh engine on a batch of 37 -- solve, then the adjoints -- is BIT-IDENTICAL (x, y, s, iters, status,
dA, dq, adj; dP with a native quadratic objective) to
  * the same instances solved as a sub-batch of 7, and one by one (per-instance templates: B = 1 legitimately leaves the shared-A path);
  * the 37 scattered inside a batch of 800 (more than the 768 workgroups of the re-solve grid; the global-residency workspaces are indexed per instance);
  * the 37 with three poisoned neighbours: a NaN and an Inf in an A value and b scaled by 1e300 -- on shared-A templates a NaN in b, an Inf in c and b scaled
    by 1e300, so that A stays shared.  The poisoned instances must not be reported solved (1) or solved / inaccurate (2); the kernels end them as -6;
  * one engine running B = 37, 800, 7, 37, 37 (the last two on other data) with the adjoints after every solve: the two-tile history, the alternating
    re-solve lists and the shared-A path's workspaces then carry state between calls, and every call must still equal a fresh engine's answer.
Adjoints: per-instance templates with a linear objective run ce_vjp with q_eval (k_backward_ns + LSQR re-solve where planned) and without it; native
quadratic objectives ce_vjp_qp; shared-A templates the shared-A LSQR adjoint (CE_CONST_A=1).
Shared-A templates whose dense rows exceed 64 (sp_RP == 0) run the batch-GEMM path of interfaces/const_a.py: it drops finished instances from its working
set, so the rocBLAS GEMM sizes -- and with them the algorithms rocBLAS picks -- depend on the batch; there floating-point outputs are compared within 1e-12
relative (integers exactly).  Not covered: plan_kit's ledger-only family zl_n_m700 (n = 440 .. 700: a batch of 800 costs minutes per call)."""
import numpy as np
import pytest
import torch

import plan_kit as pk
from cvxpylayers_amd import problems as P
from kit import TIGHT_LSQR

pytestmark = pytest.mark.gpu

SET = dict(eps=1e-8, max_iters=50000, acceleration_lookback=0)
FWD = ("fwd_mode", "f2_variant", "rt_variant", "wl", "aa_ok", "gen_blocked_f", "qp_native")
BWD = ("bwd_mode", "brt_variant", "two_tile", "ns_variant", "gen_blocked_b")
SKIP_FAMILIES = ("zl_n_m700",)
SHARED = pk.SHARED_FAMILY[0]


def representatives():
    from test_gpu_plan_edges import discovery
    _, seen, _ = discovery()
    best = {}
    for fam, v, p in seen.values():
        if fam in SKIP_FAMILIES:
            continue
        n, cones, _, pstruct = pk.shape_of(fam, v)
        size = n * P.cone_rows(cones)
        if fam == SHARED:
            keys = [("shared", p["sp_RP"])]
        else:
            kind = "qp" if pstruct is not None else "lin"
            keys = [(kind, "fwd") + tuple(p[f] for f in FWD), (kind, "bwd") + tuple(p[f] for f in BWD)]
        for k in keys:
            if k not in best or size < best[k][0]:
                best[k] = (size, fam, v)
    reps = sorted({(fam, v) for _, fam, v in best.values()})
    print(f"\nbatch purity: {len(reps)} representative shapes for {len(best)} forward / adjoint / shared-A plans: {reps}")
    return reps


class Shape:
    def __init__(self, fam, v):
        from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
        self.fam, self.v = fam, v
        self.n, self.cones, self.pat, pstruct = pk.shape_of(fam, v)
        self.m = P.cone_rows(self.cones)
        self.tpl = P.dense_template(self.n, self.cones, pattern=self.pat)
        self.shared = self.pat is not None
        probe = ConeEngine(self.tpl.indices, self.tpl.indptr, self.n, self.m, self.cones, torch.device("cuda", 0), p_structure=pstruct)
        self.plan = probe.plan()
        self.pstruct = pstruct if (pstruct is not None and probe.qp_native) else None      # (a P the kernels cannot hold: the engine serves the linear objective)
        self.exact = not (self.shared and self.plan["sp_RP"] == 0)
        if self.shared:      # the one matrix of the template (as in test_gpu_plan_edges._data): dense rows + a bound row on every variable
            rng = np.random.default_rng(v)
            self.A0 = np.where(self.pat, rng.standard_normal(self.pat.shape) / np.sqrt(self.n), 0.0)
            self.A0[self.m - self.n + np.arange(self.n), np.arange(self.n)] = -(0.5 + rng.random(self.n))
        self.tag = f"{fam} v={v} n={self.n} m={self.m}" + (f" sp_RP={self.plan['sp_RP']}" if self.shared else "") + (" +P" if self.pstruct is not None else "")

    def data(self, B, seed):
        """(A, b, c, P or None, dx, dy)"""
        rng = np.random.default_rng(seed)
        if self.shared:
            x0 = rng.standard_normal((B, self.n)) * 0.5; s0, y0 = P._interior_point(rng, self.cones, B)
            A = np.broadcast_to(self.A0, (B, self.m, self.n)).copy(); b = x0 @ self.A0.T + s0; c = -(y0 @ self.A0)
        else:
            A, b, c = P.generate(self.n, self.cones, B, seed=seed)
        Pm = None
        if self.pstruct is not None:
            F = rng.standard_normal((B, self.n, self.n)) / np.sqrt(self.n)
            Pm = F @ F.transpose(0, 2, 1) + 0.1 * np.eye(self.n)
        return A, b, c, Pm, rng.standard_normal((B, self.n)), rng.standard_normal((B, self.m))

    def engine(self):
        from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
        return ConeEngine(self.tpl.indices, self.tpl.indptr, self.n, self.m, self.cones, torch.device("cuda", 0), p_structure=self.pstruct)

    def run(self, eng, A, b, c, Pm, dx, dy):
        """solve + the adjoints of the path; every output on the host"""
        from cvxpylayers_amd.interfaces.mi355_if import make_settings
        dev = torch.device("cuda", 0)
        A_eval, q_eval = self.tpl.values_from_dense(A, b, c)
        A_bm = eng.to_batch_major(torch.from_numpy(A_eval).to(dev)); q_t = torch.from_numpy(q_eval).to(dev)
        P_bm = None
        if Pm is not None:
            idx, ptr = self.pstruct
            P_bm = torch.from_numpy(np.ascontiguousarray(Pm[:, idx, np.repeat(np.arange(self.n), np.diff(ptr))])).to(dev)
        x, y, s, iters, status, _ = eng.solve(A_bm, q_t, make_settings(dict(SET)), P_bm=P_bm)
        if self.shared:
            assert eng.last_path == "const_a", (self.tag, eng.last_path)
        dxt, dyt = torch.from_numpy(dx).to(dev), torch.from_numpy(dy).to(dev)
        out = dict(x=x, y=y, s=s, iters=iters, status=status)
        if self.shared:
            g = eng.vjp(A_bm, x, y, s, dxt, dyt, path="const_a", lsqr=TIGHT_LSQR, q_eval=q_t)
            out.update(dA=g[0].t(), dq=g[1].t(), adj=g[2])
        elif P_bm is not None:
            g = eng.vjp(A_bm, x, y, s, dxt, dyt, P_bm=P_bm)
            out.update(dA=g[0].t(), dq=g[1].t(), adj=g[2], dP=g[3])
        else:
            g1 = eng.vjp(A_bm, x, y, s, dxt, dyt, path="per_instance", lsqr=TIGHT_LSQR, q_eval=q_t)
            g2 = eng.vjp(A_bm, x, y, s, dxt, dyt, path="per_instance_dense")
            out.update(dA=g1[0].t(), dq=g1[1].t(), adj=g1[2], dA_el=g2[0].t(), dq_el=g2[1].t(), adj_el=g2[2])
        torch.cuda.synchronize()
        return {k: t.detach().cpu() for k, t in out.items()}

    def same(self, got, want, rows_got, rows_want, what):
        for k in want:
            a, b = got[k][rows_got], want[k][rows_want]
            if self.exact or not a.is_floating_point():
                ok = torch.equal(a, b)
                bad = ~(a == b).reshape(len(rows_got), -1).all(dim=1)
            else:          # (the batch-GEMM path: see the module docstring)
                err = ((a - b).abs().reshape(len(rows_got), -1).max(dim=1).values / (1 + b.abs().reshape(len(rows_got), -1).max(dim=1).values))
                bad = ~(err <= 1e-12)
                ok = not bool(bad.any())
            if not ok:
                raise AssertionError(f"{self.tag} {what}: {k} differs on instances {np.flatnonzero(bad.numpy())[:8].tolist()} (of {len(rows_got)})")


def _sel(data, idx):
    return tuple(None if t is None else np.ascontiguousarray(t[idx]) for t in data)


@pytest.fixture(scope="module")
def reps():
    return representatives()


def test_purity_over_every_plan(reps, monkeypatch):
    for fam, v in reps:
        sh = Shape(fam, v)
        with monkeypatch.context() as mp:
            if sh.shared:
                mp.setenv("CE_CONST_A", "1")
            base = sh.data(37, seed=v)
            ref = sh.run(sh.engine(), *base)
            assert np.isin(ref["status"].numpy(), (1, 2)).all(), (sh.tag, ref["status"])
            all37 = np.arange(37)
            # sub-batches
            sub = np.array([0, 5, 11, 17, 23, 29, 36])
            sh.same(sh.run(sh.engine(), *_sel(base, sub)), ref, np.arange(7), sub, "sub-batch of 7")
            if not sh.shared:
                one = np.array([13])
                sh.same(sh.run(sh.engine(), *_sel(base, one)), ref, np.arange(1), one, "single instance")
            # scattered inside 800
            big = tuple(None if t is None else t.copy() for t in sh.data(800, seed=v + 10_000))
            pos = np.sort(np.random.default_rng(v).choice(800, 37, replace=False))
            for t, bt in zip(base, big):
                if t is not None:
                    bt[pos] = t
            sh.same(sh.run(sh.engine(), *big), ref, pos, all37, "37 inside 800")
            # poisoned neighbours
            ppos = np.array([2, 19, 38])
            keep = np.setdiff1d(np.arange(40), ppos)
            pois = tuple(None if t is None else np.empty((40,) + t.shape[1:]) for t in base)
            for t, pt in zip(base, pois):
                if t is not None:
                    pt[keep] = t
                    pt[ppos] = t[:3]
            A_p, b_p, c_p = pois[:3]
            if sh.shared:
                b_p[2, 0] = np.nan
                c_p[19, -1] = np.inf
            else:
                A_p[2, 0, 0] = np.nan
                A_p[19, -1, -1] = np.inf
            b_p[38] *= 1e300
            got = sh.run(sh.engine(), *pois)
            sh.same(got, ref, keep, all37, "poisoned neighbours")
            st = got["status"][ppos].numpy()
            assert not np.isin(st, (1, 2)).any(), (sh.tag, st)
            print(f"{sh.tag}: poisoned statuses {st.tolist()}")


def test_call_history_does_not_reach_the_answer(reps, monkeypatch):
    for fam, v in reps:
        sh = Shape(fam, v)
        with monkeypatch.context() as mp:
            if sh.shared:
                mp.setenv("CE_CONST_A", "1")
            calls = [sh.data(37, seed=v), sh.data(800, seed=v + 1), sh.data(7, seed=v + 2), sh.data(37, seed=v + 3), sh.data(37, seed=v + 4)]
            eng = sh.engine()
            for i, d in enumerate(calls):
                got = sh.run(eng, *d)
                want = sh.run(sh.engine(), *d)
                B = d[0].shape[0]
                sh.same(got, want, np.arange(B), np.arange(B), f"call {i} (B = {B}) of the sequence")
