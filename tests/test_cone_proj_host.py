"""Host-side checks of the stand-alone cone projection (cvxpylayers_amd/cones.py, csrc/ce_lds_cone_proj.h, csrc/ce_cone_proj_triple.h), no GPU:
the LDS footprint and the state layout compiled with g++ as the library compiles them; the launches a cone set needs; the per-triple
forward-plus-Jacobian routine on special and non-finite points (it must RETURN, with finite or NaN outputs, before any GPU run feeds it the same inputs);
argument validation of cones.project before any device use."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from oracle import oracle
import cone_proj_kit as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cvxpylayers_amd", "csrc")

LAYOUT_SRC = r'''
#include "ce_lds_cone_proj.h"
extern "C" {
int h_lds_doubles(int k) { return cone_proj_psd_lds_doubles(k); }
int h_fits(int k) { return cone_proj_psd_fits(k) ? 1 : 0; }
int h_max_order() { return CONE_PROJ_PSD_MAX; }
int h_lds_bytes() { return CONE_PROJ_LDS_BYTES; }
// out: m, state_len, tri_state0, launch_rows, launch_psd, launch_triples, nq_small, nq_large, e_row0
int h_layout(int z, int l, int nq, const int *q, int ns, const int *s, int nep, int np, long long *out, int *qoff, int *soff, long long *sstate, int *small, int *large) {
    ConeProjLayout L;
    const int rc = cone_proj_layout(z, l, nq, q, ns, s, nep, np, &L, qoff, soff, sstate, small, large);
    if (rc) return rc;
    out[0] = L.m; out[1] = L.state_len; out[2] = L.tri_state0; out[3] = L.launch_rows; out[4] = L.launch_psd; out[5] = L.launch_triples;
    out[6] = L.nq_small; out[7] = L.nq_large; out[8] = L.e_row0;
    return 0;
}
}
'''

TRIPLE_SRC = r'''
#include <cmath>
#define __device__
#define __forceinline__ inline
#define __noinline__
using std::fmin; using std::fmax;
#include "ce_cone_proj_triple.h"
extern "C" void h_triple(const double *v, int is_exp, double a, int dual, double *out, double *J, int want_jac) {
    cone_triple_project(v, is_exp != 0, a, dual, out, want_jac ? J : nullptr);
}
'''


def _build(tmp, name, src, flags=()):
    (tmp / f"{name}.cpp").write_text(src)
    so = str(tmp / f"lib{name}.so")
    subprocess.check_call(["g++", "-O2", "-shared", "-fPIC", *flags, "-I", CSRC, "-o", so, str(tmp / f"{name}.cpp")])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    L = _build(tmp_path_factory.mktemp("cone_layout"), "cone_layout", LAYOUT_SRC, ("-D__host__=", "-D__device__="))
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    L.h_layout.argtypes = [C.c_int, C.c_int, C.c_int, ip, C.c_int, ip, C.c_int, C.c_int, lp, ip, ip, lp, ip, ip]
    return L


@pytest.fixture(scope="module")
def triple(tmp_path_factory):
    L = _build(tmp_path_factory.mktemp("cone_triple"), "cone_triple", TRIPLE_SRC)
    dp = C.POINTER(C.c_double)
    L.h_triple.argtypes = [dp, C.c_int, C.c_double, C.c_int, dp, dp, C.c_int]
    return L


def _layout(L, cones):
    q = np.asarray(cones.get("q", []), dtype=np.int32); s = np.asarray(cones.get("s", []), dtype=np.int32)
    out = np.zeros(9, dtype=np.int64); qoff = np.zeros(len(q) + 1, dtype=np.int32); soff = np.zeros(len(s) + 1, dtype=np.int32)
    sst = np.zeros(len(s) + 1, dtype=np.int64); small = np.zeros(len(q) + 1, dtype=np.int32); large = np.zeros(len(q) + 1, dtype=np.int32)
    ip, lp = C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    rc = L.h_layout(cones.get("z", 0), cones.get("l", 0), len(q), q.ctypes.data_as(ip), len(s), s.ctypes.data_as(ip), cones.get("ep", 0), len(cones.get("p", [])),
                    out.ctypes.data_as(lp), qoff.ctypes.data_as(ip), soff.ctypes.data_as(ip), sst.ctypes.data_as(lp), small.ctypes.data_as(ip), large.ctypes.data_as(ip))
    names = ("m", "state_len", "tri_state0", "launch_rows", "launch_psd", "launch_triples", "nq_small", "nq_large", "e_row0")
    return rc, dict(zip(names, out.tolist())), qoff, soff, sst[:len(s)], small, large


def test_state_offsets_are_disjoint_and_sum_to_the_state_length(layout):
    cones = {"z": 2, "l": 3, "q": [3, 17], "s": [3, 5, 40, 1], "ep": 2, "p": [0.3, -0.6]}
    rc, L, qoff, soff, sst, _, _ = _layout(layout, cones)
    assert rc == 0 and L["m"] == K.rows_of(cones)
    sizes = [k * k + k for k in cones["s"]] + [9] * 4
    starts = list(sst) + [L["tri_state0"] + 9 * c for c in range(4)]
    ends = [a + n for a, n in zip(starts, sizes)]
    assert starts[0] == 0 and starts[1:] == ends[:-1] and ends[-1] == L["state_len"] == sum(sizes)      # back to back: disjoint and complete
    assert list(qoff) == [5, 8, 25] and list(soff) == [25, 31, 46, 866, 867] and L["e_row0"] == 867
    assert _layout(layout, {"l": 4, "q": [3]})[1]["state_len"] == 0          # plain cones keep no state


def test_footprint_is_monotone_and_the_stated_largest_order_is_the_last_that_fits(layout):
    kmax = layout.h_max_order()
    fp = [layout.h_lds_doubles(k) for k in range(1, kmax + 3)]
    assert all(b >= a for a, b in zip(fp, fp[1:]))
    assert kmax == 82
    assert layout.h_fits(kmax) == 1 and 8 * layout.h_lds_doubles(kmax) <= layout.h_lds_bytes() == 160 * 1024
    assert layout.h_fits(kmax + 1) == 0 and 8 * layout.h_lds_doubles(kmax + 1) > layout.h_lds_bytes()
    assert all(layout.h_fits(k) == 1 for k in range(1, kmax + 1)) and layout.h_fits(0) == 0
    assert _layout(layout, {"s": [3, kmax + 1]})[0] == 2                     # the offending block's index + 1


def test_absent_kinds_produce_no_launch(layout):
    def launches(cones):
        L = _layout(layout, cones)[1]
        return (L["launch_rows"], L["launch_psd"], L["launch_triples"])
    assert launches({"l": 3}) == (1, 0, 0) and launches({"z": 1}) == (1, 0, 0) and launches({"q": [3]}) == (1, 0, 0)
    assert launches({"s": [4]}) == (0, 1, 0) and launches({"ep": 1}) == (0, 0, 1) and launches({"p": [0.5]}) == (0, 0, 1)
    assert launches({"z": 1, "s": [2], "p": [0.2]}) == (1, 1, 1)
    L = _layout(layout, {"q": [16, 17, 3, 64]})
    assert (L[1]["nq_small"], L[1]["nq_large"]) == (2, 2) and list(L[5][:2]) == [0, 2] and list(L[6][:2]) == [1, 3]


def test_project_validates_its_arguments_before_any_device_use():
    from cvxpylayers_amd import cones
    from cvxpylayers_amd.interfaces import project
    assert project is cones.project
    v = torch.zeros(4, 3, dtype=torch.float64)
    with pytest.raises(ValueError, match="rows"):
        cones.project(v, {"l": 2})                           # wrong m
    with pytest.raises(ValueError, match="exponent"):
        cones.project(v, {"p": [1.0]})
    with pytest.raises(ValueError, match="exponent"):
        cones.project(v, {"p": [0.0]})
    with pytest.raises(ValueError, match="PSD order"):
        cones.project(torch.zeros(2, 1), {"s": [0]})
    with pytest.raises(TypeError, match="dict"):
        cones.project(v, [3])
    with pytest.raises(ValueError, match="unknown cone keys"):
        cones.project(v, {"l": 3, "psd": [2]})
    with pytest.raises(ValueError):
        cones.ConeProjection({"q": [0]})
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="needs a ROCm GPU; there is no CPU fallback"):
            cones.project(v, {"l": 3})


def test_an_order_beyond_the_footprint_is_refused_before_any_hip_call():
    """ce_cones_create checks the LDS footprint on the host first: the refusal needs no device and names the order and the bound"""
    from cvxpylayers_amd.interfaces.cone_set import ConeSet
    with pytest.raises(NotImplementedError, match=r"PSD order 83 .* largest supported order is 82"):
        ConeSet({"s": [4, 83]}, torch.device("cuda", 0))


def _run_triple(T, v, is_exp, a, dual, want_jac=True):
    v = np.asarray(v, dtype=np.float64); out = np.full(3, 7.0); J = np.full(9, 7.0)
    dp = C.POINTER(C.c_double)
    T.h_triple(v.ctypes.data_as(dp), int(is_exp), float(a), int(dual), out.ctypes.data_as(dp), J.ctypes.data_as(dp), int(want_jac))
    return out, J.reshape(3, 3)


KINDS = [(True, 0.0), (True, 0.0), (False, 0.3), (False, -0.6)]      # the triples of K.TRIPLES


@pytest.mark.parametrize("dual", [False, True])
def test_triple_routine_returns_on_special_and_non_finite_points(triple, dual):
    for is_exp, a in KINDS[1:]:
        for v in K.SPECIAL_TRIPLES:
            out, J = _run_triple(triple, v, is_exp, a, dual)
            ref = oracle.proj_exp(v, dual=dual) if is_exp else oracle.proj_pow(v, a, dual=dual)
            assert np.isfinite(out).all() and np.isfinite(J).all(), (v, is_exp, a)
            assert np.abs(out - ref).max() <= 1e-10 * (1 + np.linalg.norm(v)), (v, is_exp, a, out, ref)
        for v in ([np.nan, 1.0, 1.0], [np.inf, 1.0, 1.0], [1.0, -np.inf, 0.0], [0.0, 1.0, np.nan]):
            out, J = _run_triple(triple, v, is_exp, a, dual)
            assert np.isnan(out).all() and np.isnan(J).all(), (v, is_exp, a)
            out, J = _run_triple(triple, v, is_exp, a, dual, want_jac=False)
            assert np.isnan(out).all() and (J == 7.0).all()


@pytest.mark.parametrize("dual", [False, True])
def test_triple_routine_matches_the_oracle(triple, dual):
    rng = np.random.default_rng(5)
    v = K.triple_points(rng, 200).reshape(200, 4, 3)
    for c, (is_exp, a) in enumerate(KINDS):
        for i in range(200):
            w = v[i, c]
            out, J = _run_triple(triple, w, is_exp, a, dual)
            ref = oracle.proj_exp(w, dual=dual) if is_exp else oracle.proj_pow(w, a, dual=dual)
            Jr = oracle.dproj_exp(w, dual=dual) if is_exp else oracle.dproj_pow(w, a, dual=dual)
            assert np.abs(out - ref).max() <= 1e-12 * (1 + np.linalg.norm(w)), (w, is_exp, a)
            assert np.abs(J - Jr).max() <= (1e-8 if is_exp else 1e-6), (w, is_exp, a)
