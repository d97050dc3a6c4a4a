"""The served class, the row selection and the LDS footprint of k_fwd_wave (cvxpylayers_amd/csrc/ce_lds_fwd_wave.h, ce_variants_wave.h) are plain C++ apart from their
qualifiers: the kernel carves with them and ce_create selects with them, so they are checked here on the host, compiled with g++:
  * served and refused templates, the first-fit row at every instantiation's bounds and one past them;
  * the footprint: positive, 8-aligned, within the device limit the other footprints use (160 KB), equal to the kernel's carve written out;
  * memory safety: a stand-alone program (its own main, nothing loaded into python) built with -fsanitize=address,undefined walks n = 1 .. 40 x m = 1 .. 72 through
    both functions, exits 0 and prints what the shared object returns."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cvxpylayers_amd", "csrc")
LDS_LIMIT = 160 * 1024
SRC = r'''
#include <cstddef>
#include <cstdio>
#define __host__
#define __device__
#include "ce_lds_fwd_wave.h"
#define X(V, NX, MY, WPS) {V, NX, MY, WPS},
static const int ROWS[][4] = {CE_WAVE_VARIANTS(X)};
#undef X
extern "C" {
int h_rows() { return (int)(sizeof ROWS / sizeof ROWS[0]); }
void h_row(int v, int *out) { for (int k = 0; k < 4; k++) out[k] = ROWS[v][k]; }
int h_variant(int n, int m, int z, int l, int nq, const int *q, int ns, int nep, int np, int nnz_p) { return fwd_wave_variant(n, m, z, l, nq, q, ns, nep, np, nnz_p); }
long h_lds(int v, int n, int m) { return (long)fwd_wave_lds_bytes(v, n, m); }
const char *h_refusal(int n, int m, int ns, int nep, int np, int nnz_p) { return fwd_wave_refusal(n, m, ns, nep, np, nnz_p); }
}
#ifdef WAVE_WALK_MAIN
// every (n, m) of the grid as: all rows nonnegative; one second-order cone over all rows; z = 1 and cones of 1 and m - 2 rows (m >= 3)
int main() {
    for (int n = 1; n <= 40; n++)
        for (int m = 1; m <= 72; m++) {
            int q1[1] = {m}, q2[2] = {1, m - 2};
            const int va = fwd_wave_variant(n, m, 0, m, 0, nullptr, 0, 0, 0, 0), vb = fwd_wave_variant(n, m, 0, 0, 1, q1, 0, 0, 0, 0);
            const int vc = m >= 3 ? fwd_wave_variant(n, m, 1, 0, 2, q2, 0, 0, 0, 0) : va;
            long lds[4];
            for (int v = -1; v < 3; v++) lds[v + 1] = (long)fwd_wave_lds_bytes(v, n, m);
            printf("%d %d %d %d %d %ld %ld %ld %ld\n", n, m, va, vb, vc, lds[0], lds[1], lds[2], lds[3]);
        }
    return 0;
}
#endif
'''


def _build(d, program=False, extra=()):
    (d / "host.cpp").write_text(SRC)
    out = str(d / ("wave_walk" if program else "libwave_host.so"))
    mode = ["-DWAVE_WALK_MAIN"] if program else ["-shared", "-fPIC"]
    subprocess.check_call(["g++", "-std=c++17", "-O1", *mode, *extra, "-I", CSRC, "-o", out, str(d / "host.cpp")])
    return out


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    L = C.CDLL(_build(tmp_path_factory.mktemp("wave_host")))
    L.h_variant.argtypes = [C.c_int] * 5 + [C.POINTER(C.c_int)] + [C.c_int] * 4
    L.h_lds.restype = C.c_long; L.h_lds.argtypes = [C.c_int] * 3
    L.h_row.argtypes = [C.c_int, C.POINTER(C.c_int)]
    L.h_refusal.restype = C.c_char_p; L.h_refusal.argtypes = [C.c_int] * 6
    return L


def _rows(host):
    rows = []
    for v in range(host.h_rows()):
        buf = (C.c_int * 4)()
        host.h_row(v, buf)
        rows.append(tuple(buf))
    return rows


def _variant(host, n, m, z=0, l=None, q=(), ns=0, nep=0, np_=0, nnz_p=0):
    q = list(q)
    l = m - z - sum(q) if l is None else l
    arr = (C.c_int * max(len(q), 1))(*q)
    return host.h_variant(n, m, z, l, len(q), arr, ns, nep, np_, nnz_p)


def test_variant_list_is_ordered_and_within_one_wave(host):
    rows = _rows(host)
    assert [r[0] for r in rows] == list(range(len(rows))) and len(rows) >= 1
    for (_, nx, my, wps), nxt in zip(rows, rows[1:] + [None]):
        assert 8 <= nx <= 32 and my <= 64 and 64 % nx == 0 and 64 % my == 0 and 1 <= wps <= 8
        if nxt is not None:
            assert nxt[1] >= nx and nxt[2] >= my and (nxt[1], nxt[2]) != (nx, my)      # first fit walks towards larger bounds
    assert rows[-1][1:3] == (32, 64)
    # the list lives in a header of its own, not in ce_variants.h
    assert "CE_WAVE_VARIANTS" not in open(os.path.join(CSRC, "ce_variants.h")).read()
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "ce_tu_fwd_wave.hip" in mk and "$(OBJDIR)/fwd_wave.o" in mk.split("OBJS")[1].split("all:")[0]


def test_served_and_refused_templates(host):
    for n, m in ((1, 1), (2, 3), (32, 64)):
        assert _variant(host, n, m) >= 0, (n, m)
    assert _variant(host, 32, 64, q=[64]) >= 0 and _variant(host, 3, 6, z=1, q=[1, 3]) >= 0
    assert _variant(host, 33, 64) == -1 and b"n > 32" in host.h_refusal(33, 64, 0, 0, 0, 0)
    assert _variant(host, 32, 65) == -1 and b"m > 64" in host.h_refusal(32, 65, 0, 0, 0, 0)
    assert _variant(host, 4, 6, l=3, ns=1) == -1 and b"PSD" in host.h_refusal(4, 6, 1, 0, 0, 0)
    assert _variant(host, 4, 6, l=3, nep=1) == -1 and b"exponential" in host.h_refusal(4, 6, 0, 1, 0, 0)
    assert _variant(host, 4, 6, l=3, np_=1) == -1 and b"power" in host.h_refusal(4, 6, 0, 0, 1, 0)
    assert _variant(host, 4, 6, nnz_p=4) == -1 and b"P structure" in host.h_refusal(4, 6, 0, 0, 0, 4)
    assert _variant(host, 4, 6, l=2) == -1          # cone rows that do not add up to m


def test_first_fit_at_every_rows_bounds_and_one_past(host):
    rows = _rows(host)
    for v, nx, my, _ in rows:
        assert _variant(host, nx, my) == v and _variant(host, 1, my) <= v and _variant(host, nx, 1) <= v
        prev = rows[v - 1] if v else None
        if prev is not None:          # one past the row before: this row (or a later one) takes over
            assert _variant(host, prev[1] + 1, 1) >= v or prev[1] == nx
            assert _variant(host, 1, prev[2] + 1) >= v or prev[2] == my
        past_n, past_m = _variant(host, nx + 1, my), _variant(host, nx, my + 1)
        assert past_n == (-1 if nx == 32 else past_n) and (past_n == -1 or past_n > v)
        assert past_m == (-1 if my == 64 else past_m) and (past_m == -1 or past_m > v)
    for n in range(1, 33):
        for m in range(1, 65):
            v = _variant(host, n, m)
            assert v == next(r[0] for r in rows if n <= r[1] and m <= r[2]), (n, m, v)


def test_footprint(host):
    rows = _rows(host)
    for n in range(1, 33):
        for m in range(1, 65):
            v = _variant(host, n, m)
            by = host.h_lds(v, n, m)
            _, nx, my, _ = rows[v]
            assert by > 0 and by % 8 == 0 and by <= LDS_LIMIT, (n, m, by)
            assert by == 8 * ((m + n) * (nx + 1) + 2 * nx + 2 * my), (n, m, by)          # A-hat, G, two x and two y staging vectors
            assert host.h_lds(v, nx + 1, m) == 0 and host.h_lds(v, n, my + 1) == 0 and host.h_lds(-1, n, m) == 0 and host.h_lds(len(rows), n, m) == 0
    assert host.h_lds(len(rows) - 1, 32, 64) == 8 * (96 * 33 + 64 + 128) == 26880
    # the carve of the kernel is the footprint's terms in the footprint's order
    src = open(os.path.join(CSRC, "ce_forward_wave.h")).read()
    assert re.search(r"\*A = sm, \*G = A \+ m \* LD, \*xb = G \+ n \* LD, \*xb2 = xb \+ NX, \*yb = xb2 \+ NX, \*yb2 = yb \+ MY;", src)


def test_host_unit_under_sanitizers(tmp_path, host):
    exe = _build(tmp_path, program=True, extra=["-g", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    lines = [tuple(int(x) for x in ln.split()) for ln in run.stdout.splitlines()]
    assert len(lines) == 40 * 72
    for n, m, va, vb, vc, *lds in lines:
        assert va == vb == _variant(host, n, m) and vb == _variant(host, n, m, q=[m])
        assert vc == (_variant(host, n, m, z=1, q=[1, m - 2]) if m >= 3 else va)
        assert (va >= 0) == (n <= 32 and m <= 64)
        assert lds == [host.h_lds(v, n, m) for v in range(-1, 3)]
