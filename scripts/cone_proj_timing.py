"""Times of the stand-alone cone projection and its derivative (ce_cone_project with state, ce_cone_dproject) next to three yardsticks, in one process:
  (a) the same maps written as torch ops (clamp, norms, torch.linalg.eigh plus matmuls; the derivative from the saved decomposition) -- the new op must not be
      slower at any shape (ranges must not overlap on the slow side);
  (b) for the plain / second-order shapes at the large batches: achieved bytes per second from the algorithmic bytes (16 B per row for Pi, 24 B for D Pi)
      beside ce_transpose of an array of the same size, this project's streaming yardstick;
  (c) for {"s": [20]}: ce_ca_psd_mfma cold (warm = 0) on the same blocks, which runs the same sweeps.
Every call goes into buffers allocated beforehand; HIP events on the launch stream around each call, warm-up calls first, then --reps timed calls, interleaved.
Exponential / power triples have no torch closed form: their times are recorded alone.  Prints one JSON line; --out also writes it to a file.

    python scripts/cone_proj_timing.py [--reps 30] [--warmup 5] [--out profiles/cones/cone_proj.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cvxpylayers_amd import _lib  # noqa: E402
from cvxpylayers_amd import problems as P  # noqa: E402
from cvxpylayers_amd.cones import smat, svec  # noqa: E402
from cvxpylayers_amd.interfaces.cone_set import ConeSet  # noqa: E402
from cvxpylayers_amd.interfaces.mi355_if import ConeEngine  # noqa: E402

SHAPES = [("metric_4096", {"l": 20, "q": [10] * 8}, 4096), ("metric_262144", {"l": 20, "q": [10] * 8}, 262144), ("soc3_1048576", {"q": [3]}, 1048576),
          ("psd20_1024", {"s": [20]}, 1024), ("psd3_65536", {"s": [3]}, 65536), ("exp24_4096", {"ep": 24}, 4096)]
DEV = torch.device("cuda", 0)
F64 = dict(dtype=torch.float64, device=DEV)


def _soc_views(v, l, dims):
    off, out = l, []
    for d in dims:
        out.append(v[:, off:off + d]); off += d
    return out


def torch_rows_soc(v, l, dims):
    parts = [v[:, :l].clamp(min=0)]
    if dims and len(set(dims)) == 1:          # equal cones: one batched expression, the fair torch version
        d = dims[0]
        c = v[:, l:].reshape(v.shape[0], len(dims), d)
        t, z = c[..., :1], c[..., 1:]
        nz = z.norm(dim=-1, keepdim=True)
        lam = torch.where(nz <= t, 1.0, torch.where(nz <= -t, 0.0, (t + nz) / (2 * nz)))
        parts.append(torch.cat([torch.where(nz <= t, t, lam * nz), lam * z], dim=-1).reshape(v.shape[0], -1))
    return torch.cat(parts, dim=1)


def torch_rows_soc_d(v, h, l, dims):
    parts = [torch.where(v[:, :l] > 0, h[:, :l], 0.0)]
    if dims:
        d = dims[0]
        c, g = v[:, l:].reshape(v.shape[0], len(dims), d), h[:, l:].reshape(v.shape[0], len(dims), d)
        t, z, gt, gz = c[..., :1], c[..., 1:], g[..., :1], g[..., 1:]
        nz = z.norm(dim=-1, keepdim=True)
        u = (z * gz).sum(dim=-1, keepdim=True) / nz
        lam = (t + nz) / (2 * nz)
        mid = torch.cat([0.5 * (gt + u), lam * gz + 0.5 * (gt - t * u / nz) / nz * z], dim=-1)
        parts.append(torch.where(nz <= t, g, torch.where(nz <= -t, 0.0, mid)).reshape(v.shape[0], -1))
    return torch.cat(parts, dim=1)


def torch_psd(S):
    w, V = torch.linalg.eigh(S)
    return (V * w.clamp(min=0).unsqueeze(-2)) @ V.transpose(-1, -2), w, V


def torch_psd_d(w, V, H):
    p = w.clamp(min=0)
    wi, wj = w.unsqueeze(-1), w.unsqueeze(-2)
    Bm = torch.where((wi > 0) & (wj > 0), 1.0, torch.where((wi <= 0) & (wj <= 0), 0.0, (p.unsqueeze(-1) - p.unsqueeze(-2)) / (wi - wj)))
    return V @ (Bm * (V.transpose(-1, -2) @ H @ V)) @ V.transpose(-1, -2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default=None, help="comma-separated subset of the shape names")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cone_proj_timing.py measures on the GPU; there is nothing to fall back to")
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    tcones = {"z": 1, "l": 2, "q": [3], "s": [20]}                    # an engine for ce_transpose and ce_ca_psd_mfma (order-20 block behind 6 plain rows)
    tpl = P.dense_template(3, tcones)
    eng = ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tcones, DEV)
    res = dict(reps=a.reps, warmup=a.warmup, shapes={})
    slower = []
    for name, cones, B in SHAPES:
        if a.shapes and name not in a.shapes.split(","):
            continue
        cs = ConeSet(cones, DEV)
        m = cs.m
        gen = torch.Generator(device=DEV); gen.manual_seed(1)
        v = torch.randn((B, m), generator=gen, **F64); h = torch.randn((B, m), generator=gen, **F64)
        out, dout = torch.empty((B, m), **F64), torch.empty((B, m), **F64)
        state = torch.empty((B, max(cs.state_len, 1)), **F64)
        sp = state.data_ptr() if cs.state_len else None

        def project():
            _lib.check(L.ce_cone_project(cs._h, B, v.data_ptr(), m, 0, out.data_ptr(), m, sp, st), "ce_cone_project")

        def dproject():
            _lib.check(L.ce_cone_dproject(cs._h, B, v.data_ptr(), m, 0, sp, h.data_ptr(), m, dout.data_ptr(), m, st), "ce_cone_dproject")
        calls = [("project", project), ("dproject", dproject)]
        l, dims, orders = cones.get("l", 0), cones.get("q", []), cones.get("s", [])
        check = None
        if orders:
            k = orders[0]
            S, Hm = smat(v, k), smat(h, k)
            wV = {}

            def t_project():
                X, wV["w"], wV["V"] = torch_psd(S)
                return X

            def t_dproject():
                return torch_psd_d(wV["w"], wV["V"], Hm)
            calls += [("torch_project", t_project), ("torch_dproject", t_dproject)]
            check = lambda: (svec(t_project()), svec(t_dproject()))      # noqa: E731
            if k == 20:
                lfull = tpl.n + tpl.m + 1; lp = lfull + (lfull & 1); off = tpl.n + 6
                U = torch.zeros((B, lp), **F64); Vst = torch.zeros((B, 1, k * k), **F64); active = torch.ones(B, dtype=torch.int32, device=DEV)

                def ca_psd_mfma_cold():
                    U[:, off:off + m] = v          # (the call projects in place: the copy is inside the bracket, 1.7 MB at B = 1024)
                    _lib.check(L.ce_ca_psd_mfma(eng._h, B, lp, U.data_ptr(), Vst.data_ptr(), 0, active.data_ptr(), st), "ce_ca_psd_mfma")
                calls.append(("ce_ca_psd_mfma_cold", ca_psd_mfma_cold))
        elif l or dims:
            calls += [("torch_project", lambda: torch_rows_soc(v, l, dims)), ("torch_dproject", lambda: torch_rows_soc_d(v, h, l, dims))]
            check = lambda: (torch_rows_soc(v, l, dims), torch_rows_soc_d(v, h, l, dims))      # noqa: E731
            tr_out = torch.empty(B * m, **F64)

            def transpose():
                _lib.check(L.ce_transpose(eng._h, B, m, v.data_ptr(), tr_out.data_ptr(), st), "ce_transpose")
            calls.append(("transpose", transpose))
        times = {n_: [] for n_, _ in calls}
        for it in range(a.warmup + a.reps):
            for n_, fn in calls:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); fn(); e1.record(); e1.synchronize()
                if it >= a.warmup:
                    times[n_].append(e0.elapsed_time(e1))
        r = dict(cones={k_: (v_ if not isinstance(v_, list) or len(v_) < 4 else f"[{v_[0]}] * {len(v_)}") for k_, v_ in cones.items()}, B=B, rows=m)
        for n_, _ in calls:
            t = np.asarray(times[n_])
            r[n_] = dict(ms_median=float(np.median(t)), ms_min=float(t.min()), ms_max=float(t.max()))
        if check is not None:                                       # the yardstick computed the same thing
            tp, td = check()
            r["max_abs_diff_project_vs_torch"] = float((out - tp).abs().max()); r["max_abs_diff_dproject_vs_torch"] = float((dout - td).abs().max())
            for mine, theirs in (("project", "torch_project"), ("dproject", "torch_dproject")):
                r[f"ratio_torch_over_{mine}"] = r[theirs]["ms_median"] / r[mine]["ms_median"]
                if r[mine]["ms_max"] > r[theirs]["ms_min"] and r[mine]["ms_median"] > r[theirs]["ms_median"]:
                    slower.append(f"{name}:{mine}")
        if "transpose" in r:
            for mine, per_row in (("project", 16.0), ("dproject", 24.0)):
                r[mine].update(bytes_needed=per_row * B * m, tb_per_s_at_median=per_row * B * m / (r[mine]["ms_median"] * 1e-3) / 1e12)
            r["transpose"].update(bytes_needed=16.0 * B * m, tb_per_s_at_median=16.0 * B * m / (r["transpose"]["ms_median"] * 1e-3) / 1e12)
            r["ratio_project_bandwidth_over_transpose"] = r["project"]["tb_per_s_at_median"] / r["transpose"]["tb_per_s_at_median"]
            r["ratio_dproject_bandwidth_over_transpose"] = r["dproject"]["tb_per_s_at_median"] / r["transpose"]["tb_per_s_at_median"]
        if "ce_ca_psd_mfma_cold" in r:
            r["ratio_project_over_ce_ca_psd_mfma_cold"] = r["project"]["ms_median"] / r["ce_ca_psd_mfma_cold"]["ms_median"]
        res["shapes"][name] = r
        del cs
    res["slower_than_torch"] = slower
    res["note"] = ("events on the launch stream around one call each; project writes the derivative state (PSD: k^2 + k doubles per block, triples: 9); torch_project of "
                   "a PSD shape is eigh plus the products on matrices already unpacked, torch_dproject starts from the saved decomposition; torch allocations are inside "
                   "the brackets, as they are in use")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if slower:
        raise SystemExit("slower than the torch ops at: " + ", ".join(slower))


if __name__ == "__main__":
    main()
