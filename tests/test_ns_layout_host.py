"""The LDS layout of k_backward_ns (cvxpylayers_amd/csrc/ce_ns_layout.h) is plain C++ apart from its qualifiers: the kernel takes every pointer from it and the
launch plan takes its total, so its invariants are checked here on the host, compiled with g++, for every row of CE_NS_VARIANTS with and without the dense P:
segments are disjoint apart from the declared members of the union region, every double segment is 8-byte aligned (the union region 16: the sweep reads it with
128-bit loads), the footprint is the end of the last segment, and the two footprints that the profile tables quote are reproduced."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kind: 0 doubles, 1 ints; role: 0 a segment of its own, 1 .. 3 a member of the union region U alive in phase 1 (a_z, publication buffers), 2 (the sweep's row
# buffers), 3 (q, g): members of one phase are disjoint, members of different phases share storage
SEGMENTS = [("A", 0, 0), ("vv", 0, 0), ("dv", 0, 0), ("rx", 0, 0), ("fvec", 0, 0), ("dB", 0, 0), ("cinfo", 0, 0), ("tvec", 0, 0), ("wgt", 0, 0), ("red", 0, 0),
            ("qaz", 0, 0), ("U", 0, 0), ("az", 0, 1), ("pub", 0, 1), ("Rbuf", 0, 2), ("qv2", 0, 3), ("mu", 0, 3),
            ("rkind", 1, 0), ("eqrow", 1, 0), ("ckind", 1, 0), ("ceq", 1, 0), ("cbase", 1, 0), ("erow", 1, 0), ("pcol", 1, 0), ("cmap", 1, 0), ("fcol", 1, 0),
            ("wrow", 1, 0), ("wsrc", 1, 0), ("wcnt", 1, 0), ("misc", 1, 0), ("Pm", 0, 0), ("ptv", 0, 0), ("peq", 1, 0), ("slack", 1, 0)]
SRC = r'''
#include <cstddef>
#define __host__
#define __device__
#include "ce_ns_layout.h"
#include "ce_variants.h"
#define X(V, NTILE, NTHR) {NTILE, NTHR},
static const int ROWS[][2] = {CE_NS_VARIANTS(X)};
#undef X
extern "C" {
int h_rows() { return (int)(sizeof ROWS / sizeof ROWS[0]); }
void h_row(int v, int *ntile, int *nthr) { *ntile = ROWS[v][0]; *nthr = ROWS[v][1]; }
// out[2 k], out[2 k + 1]: first byte and byte count of segment k in the order of SEGMENTS; returns the footprint
long h_layout(int n, int m, int nq, int ntile, int nthr, int qp, long *out) {
    const NsLayout L = ns_layout(n, m, nq, ntile, nthr, qp != 0);
    int k = 0;
#define D(s) out[k++] = 8L * L.s.off; out[k++] = 8L * L.s.len;
#define I(s) out[k++] = 4L * L.s.off; out[k++] = 4L * L.s.len;
    SEGMENT_LIST
#undef D
#undef I
    return (long)L.bytes;
}
long h_bytes(int n, int m, int nq, int ntile, int nthr, int qp) { return (long)(qp ? bwd_ns_qp_lds_bytes_of(n, m, nq, ntile, nthr) : bwd_ns_lds_bytes_of(n, m, nq, ntile, nthr)); }
}
'''


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    d = tmp_path_factory.mktemp("ns_layout")
    seg_list = " ".join(f"{'I' if kind else 'D'}({name})" for name, kind, _ in SEGMENTS)
    (d / "host.cpp").write_text(SRC.replace("SEGMENT_LIST", seg_list))
    so = str(d / "libns_layout_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-shared", "-fPIC", "-I", os.path.join(ROOT, "cvxpylayers_amd", "csrc"), "-o", so, str(d / "host.cpp")])
    L = C.CDLL(so)
    L.h_layout.restype = C.c_long; L.h_layout.argtypes = [C.c_int] * 6 + [C.POINTER(C.c_long)]
    L.h_bytes.restype = C.c_long; L.h_bytes.argtypes = [C.c_int] * 6
    L.h_row.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    return L


def _rows(host):
    rows = []
    for v in range(host.h_rows()):
        a, b = C.c_int(), C.c_int()
        host.h_row(v, C.byref(a), C.byref(b))
        rows.append((a.value, b.value))
    return rows


def _check(host, n, m, nq, ntile, nthr, qp):
    buf = (C.c_long * (2 * len(SEGMENTS)))()
    total = host.h_layout(n, m, nq, ntile, nthr, qp, buf)
    case = (n, m, nq, ntile, nthr, qp)
    seg = {name: (buf[2 * k], buf[2 * k] + buf[2 * k + 1], kind, role) for k, (name, kind, role) in enumerate(SEGMENTS)}
    assert total == host.h_bytes(n, m, nq, ntile, nthr, qp), case
    for name, (b0, b1, kind, role) in seg.items():
        assert 0 <= b0 <= b1 <= total, (case, name)
        if b1 > b0:
            assert b0 % (4 if kind else 8) == 0, (case, name)
    assert seg["U"][0] % 16 == 0, case
    if not qp:
        assert all(seg[s][0] == seg[s][1] for s in ("Pm", "ptv", "peq")), case
    # the segments of their own tile the footprint: sorted by first byte, none overlaps its successor, gaps are alignment only, the last one ends at the total
    own = sorted((b0, b1, name) for name, (b0, b1, kind, role) in seg.items() if role == 0 and b1 > b0)
    assert own[0][0] == 0 and own[-1][1] == total, case
    for (a0, a1, an), (c0, c1, cn) in zip(own, own[1:]):
        assert a1 <= c0 < a1 + 16, (case, an, cn)
    # members of the union region lie inside it; members of one phase are disjoint
    u0, u1 = seg["U"][:2]
    for phase in (1, 2, 3):
        mem = sorted((b0, b1, name) for name, (b0, b1, kind, role) in seg.items() if role == phase)
        assert mem and all(u0 <= b0 <= b1 <= u1 for b0, b1, _ in mem), (case, phase)
        for (a0, a1, an), (c0, c1, cn) in zip(mem, mem[1:]):
            assert a1 <= c0, (case, an, cn)
    assert max(b1 for name, (b0, b1, kind, role) in seg.items() if role) == u1, case          # (the union is as large as its largest phase, no larger)


def test_layout_invariants_on_a_grid(host):
    """n in 1 .. 112, m in 1 .. 260 (thinned, with both parities and the ends), nq in {0, 1, 3, m / 4}, every row of CE_NS_VARIANTS, with and without P"""
    ns = sorted(set(list(range(1, 113, 9)) + list(range(2, 113, 14)) + [31, 32, 33, 63, 64, 65, 108, 111, 112]))
    ms = sorted(set(list(range(1, 261, 23)) + list(range(2, 261, 34)) + [3, 4, 100, 259, 260]))
    count = 0
    for ntile, nthr in _rows(host):
        for n in ns:
            for m in ms:
                for nq in sorted({0, 1, 3, m // 4}):
                    for qp in (0, 1):
                        _check(host, n, m, nq, ntile, nthr, qp)
                        count += 1
    assert count > 10000


def test_quoted_footprints(host):
    """(n = 50, m = 100, no second-order cone, 4 tiles, 256 threads): 52,496 bytes, 73,096 with the dense P (profiles/jvp/k_backward_ns_qp_metadata.md)"""
    assert host.h_bytes(50, 100, 0, 4, 256, 0) == 52496
    assert host.h_bytes(50, 100, 0, 4, 256, 1) == 73096
