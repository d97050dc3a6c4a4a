"""Times of the optimal value and its envelope-theorem gradients (ce_value, ce_value_vjp in both dA layouts) at the metric configuration, next to what they
replace and to the layout pass they must not exceed, in one process at the same point (the solution at --eps):
  * ce_vjp with the cotangent dx = c, dy = 0 -- the adjoint route of  loss = c^T x  (its dc gets + x from autograd on top);
  * the same formulas as torch ops (gathers by the structure's row / column index, products, a row sum);
  * ce_transpose of a (B, nnz_aug) array: ce_value_vjp (batch-major) writes B nnz_aug doubles once, the transpose reads and writes them.
Every call goes through the C ABI into buffers allocated beforehand (no allocator in the timed region); HIP events on the launch stream around each call, warm-up
calls first, then --reps timed calls each, interleaved so that clock drift hits all.  Prints one JSON line (median, min, max in ms; achieved bytes per second of
the streaming calls from the bytes the formulas need); --out also writes it to a file.  The ONE condition: value_vjp_batch_major <= transpose (medians).

    python scripts/value_timing.py [--B 4096] [--reps 30] [--warmup 5] [--eps 1e-8] [--out profiles/value/value_M.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cvxpylayers_amd import _lib  # noqa: E402
from cvxpylayers_amd import problems as P  # noqa: E402
from cvxpylayers_amd.interfaces.mi355_if import ConeEngine, make_settings  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=P.CONFIGS["M"]["B"])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eps", type=float, default=1e-8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("value_timing.py measures on the GPU; there is nothing to fall back to")
    cfg = P.CONFIGS["M"]; n, cones, B = cfg["n"], cfg["cones"], a.B
    tpl = P.dense_template(n, cones)
    m, K = tpl.m, tpl.nnz_aug
    A, b, c = P.generate(n, cones, B, seed=11)
    A_eval, q_eval = tpl.values_from_dense(A, b, c)
    dev = torch.device("cuda", 0)
    eng = ConeEngine(tpl.indices, tpl.indptr, n, m, cones, dev)
    A_bm = torch.from_numpy(A_eval).to(dev).t().contiguous(); q_t = torch.from_numpy(q_eval).to(dev)
    x, y, s, _, status, _ = eng.solve(A_bm, q_t, make_settings(dict(eps=a.eps, acceleration_lookback=0, max_iters=100000)))
    assert (status == 1).all()
    L, h, st = _lib.lib(), eng._h, eng._stream()
    f64 = dict(dtype=torch.float64, device=dev)
    g = torch.ones(B, **f64)
    pobj, dobj = torch.empty(B, **f64), torch.empty(B, **f64)
    dA_bm, dA_min, dA_adj, tr_out = (torch.empty(B * K, **f64) for _ in range(4))
    dq_bm, dq_min, dq_adj = (torch.empty((n + 1) * B, **f64) for _ in range(3))
    adj = torch.empty(B, dtype=torch.int32, device=dev)
    dx = q_t[:n].t().contiguous(); dy = torch.zeros((B, m), **f64)
    rows = torch.from_numpy(np.asarray(tpl.indices, dtype=np.int64)).to(dev)
    cols = torch.from_numpy(np.repeat(np.arange(n + 1), np.diff(tpl.indptr)).astype(np.int64)).to(dev)
    ones = torch.ones((B, 1), **f64)

    def value():
        _lib.check(L.ce_value(h, B, A_bm.data_ptr(), 1, K, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), None, None, None, 0,
                              x.data_ptr(), y.data_ptr(), pobj.data_ptr(), dobj.data_ptr(), st), "ce_value")

    def vjp_major():
        _lib.check(L.ce_value_vjp(h, B, x.data_ptr(), y.data_ptr(), g.data_ptr(), None, dA_bm.data_ptr(), 1, K, dq_bm.data_ptr(), 1, n + 1, None, None, None, 0, st), "ce_value_vjp")

    def vjp_minor():
        _lib.check(L.ce_value_vjp(h, B, x.data_ptr(), y.data_ptr(), g.data_ptr(), None, dA_min.data_ptr(), B, 1, dq_min.data_ptr(), B, 1, None, None, None, 0, st), "ce_value_vjp")

    def adjoint():
        _lib.check(L.ce_vjp(h, B, A_bm.data_ptr(), 1, K, q_t.data_ptr(), q_t.stride(0), q_t.stride(1), x.data_ptr(), y.data_ptr(), s.data_ptr(), dx.data_ptr(), dy.data_ptr(),
                            dA_adj.data_ptr(), 1, K, dq_adj.data_ptr(), B, 1, adj.data_ptr(), st), "ce_vjp")

    def torch_ops():
        xc = torch.cat([x, ones], dim=1)
        return (q_t[:n].t() * x).sum(dim=1) + q_t[n], -(g[:, None] * y).index_select(1, rows) * xc.index_select(1, cols), g[:, None] * xc

    def transpose():
        _lib.check(L.ce_transpose(h, B, K, dA_bm.data_ptr(), tr_out.data_ptr(), st), "ce_transpose")
    calls = (("value", value), ("value_vjp_batch_major", vjp_major), ("value_vjp_batch_minor", vjp_minor), ("adjoint_route_ce_vjp", adjoint),
             ("torch_ops", torch_ops), ("transpose", transpose))
    times = {name: [] for name, _ in calls}
    for k in range(a.warmup + a.reps):
        for name, fn in calls:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); fn(); e1.record(); e1.synchronize()
            if k >= a.warmup:
                times[name].append(e0.elapsed_time(e1))
    # the calls computed the same things
    assert torch.equal(dA_bm.view(B, K), dA_min.view(K, B).t()) and torch.equal(dq_bm.view(B, n + 1), dq_min.view(n + 1, B).t())
    v_t, dA_t, dq_t = torch_ops()
    assert torch.allclose(pobj, v_t, rtol=1e-12, atol=1e-12) and torch.allclose(dA_bm.view(B, K), dA_t, rtol=1e-14, atol=0) and torch.equal(dq_bm.view(B, n + 1), dq_t)
    ok = (adj == 0)
    rel = ((dA_adj.view(B, K) - dA_bm.view(B, K)).abs().amax(dim=1) / dA_bm.view(B, K).abs().amax(dim=1))[ok]
    res = dict(config="M", B=B, n=n, m=m, nnz_aug=K, eps=a.eps, reps=a.reps, warmup=a.warmup,
               adjoint_route_regular_share=float(ok.double().mean()), adjoint_route_max_rel_diff_of_dA=float(rel.max()))
    need = dict(value=8.0 * B * (n + m + (n + 1) + m + 2), value_vjp_batch_major=8.0 * B * (K + (n + 1) + n + m + 1),
                value_vjp_batch_minor=8.0 * B * (K + (n + 1) + n + m + 1), transpose=16.0 * B * K)
    for name, _ in calls:
        t = np.asarray(times[name])
        res[name] = dict(ms_median=float(np.median(t)), ms_min=float(t.min()), ms_max=float(t.max()))
        if name in need:
            res[name].update(bytes_needed=need[name], tb_per_s_at_median=need[name] / (float(np.median(t)) * 1e-3) / 1e12)
    res["ratio_value_vjp_batch_major_over_transpose"] = res["value_vjp_batch_major"]["ms_median"] / res["transpose"]["ms_median"]
    res["ratio_adjoint_route_over_value_vjp_batch_major"] = res["adjoint_route_ce_vjp"]["ms_median"] / res["value_vjp_batch_major"]["ms_median"]
    res["condition_value_vjp_batch_major_le_transpose"] = bool(res["value_vjp_batch_major"]["ms_median"] <= res["transpose"]["ms_median"])
    res["note"] = ("events on the launch stream around one C-ABI call each (torch_ops: the three expressions, allocations included); bytes_needed counts each "
                   "array the formulas read or write once (index arrays not counted)")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not res["condition_value_vjp_batch_major_le_transpose"]:
        raise SystemExit("ce_value_vjp (batch-major) took longer than ce_transpose of the same array")


if __name__ == "__main__":
    main()
