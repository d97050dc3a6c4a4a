"""Workload for a kernel trace of the shared-A kernels that only templates with exponential / power triples, LSMR or the forward derivative reach -- the general
instantiations k_sa_lsqr<RP, HPSD=1, HTRI=1, ...> at RP 0 / 16 / 32 -- and of k_ca_psd_mfma (the batch-GEMM forward's PSD projection).  BASELINE configs 4 / 5
run none of them.  A shared A of v dense rows + one bound row per variable + one cone with single-entry rows, B instances; run it under a kernel trace:
    rocprofv3 --kernel-trace --stats -d <dir> -- python scripts/probes/sa_general_kernels.py [B]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
os.environ["CE_CONST_A"] = "1"
import numpy as np
import torch
from cvxpylayers_amd import problems as P
from cvxpylayers_amd.interfaces.mi355_if import ConeEngine, make_settings

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
N = 48
dev = torch.device("cuda", 0)
TIGHT = (1e-12, 1e-12, 400)


def template(v, extra):
    ne = sum(k * (k + 1) // 2 for k in extra.get("s", [])) + 3 * extra.get("ep", 0)
    cones = {"z": 0, "l": v + N, "q": [], **extra}
    pat = np.zeros((v + N + ne, N), dtype=bool)
    pat[:v] = True
    pat[v + np.arange(N), np.arange(N)] = True
    pat[v + N + np.arange(ne), np.arange(ne) % N] = True
    rng = np.random.default_rng(0)
    A0 = np.where(pat, rng.standard_normal(pat.shape) / np.sqrt(N), 0.0)
    A0[v + np.arange(N), np.arange(N)] = -(0.5 + rng.random(N))
    x0 = rng.standard_normal((B, N)) * 0.5
    s0, y0 = P._interior_point(rng, cones, B)
    tpl = P.dense_template(N, cones, pattern=pat)
    A_eval, q_eval = tpl.values_from_dense(np.broadcast_to(A0, (B,) + A0.shape).copy(), x0 @ A0.T + s0, -(y0 @ A0))
    eng = ConeEngine(tpl.indices, tpl.indptr, N, tpl.m, cones, dev)
    return tpl, eng, eng.to_batch_major(torch.from_numpy(A_eval).to(dev)), torch.from_numpy(q_eval).to(dev)


for v in (3, 20):          # sp_RP 16, 32
    tpl, eng, A_bm, q_t = template(v, {"ep": 1})
    x, y, s, _, status, _ = eng.solve(A_bm, q_t, make_settings(dict(eps=1e-8, max_iters=100000, acceleration_lookback=0)))
    rng = np.random.default_rng(1)
    dx, dy = (torch.from_numpy(rng.standard_normal(tuple(t.shape))).to(dev) for t in (x, y))
    tA = torch.zeros_like(A_bm); tA[:, tpl.nnz_aug - tpl.m:] = torch.from_numpy(rng.standard_normal((B, tpl.m))).to(dev)
    tq = torch.from_numpy(rng.standard_normal(tuple(q_t.shape))).to(dev)
    for rep in range(3):
        for path in ("const_a", "per_instance_lsqr"):
            eng.vjp(A_bm, x, y, s, dx, dy, path=path, lsqr=TIGHT, q_eval=q_t)
            eng.vjp(A_bm, x, y, s, dx, dy, path=path, lsqr=TIGHT + ("full", "lsmr"), q_eval=q_t)
        for path in ("const_a", "per_instance"):
            eng.jvp(A_bm, x, y, s, tA, tq, path=path, lsqr=TIGHT, q_eval=q_t)
    torch.cuda.synchronize()
    print(f"v={v} sp_RP={eng.plan()['sp_RP']} solved {float((status == 1).float().mean()):.3f} last_sa_lsqr={eng.plan().get('last_sa_lsqr')}")
os.environ["CE_SA_FWD"] = "0"          # the batch-GEMM forward: ce_ca_psd_mfma projects the PSD block every iteration
tpl, eng, A_bm, q_t = template(3, {"s": [6]})
x, y, s, it, status, _ = eng.solve(A_bm, q_t, make_settings(dict(eps=1e-6, max_iters=2000, acceleration_lookback=0)))
torch.cuda.synchronize()
print(f"batch-GEMM forward ({eng.last_const_a_kernel}): iterations mean {float(it.float().mean()):.0f}")
