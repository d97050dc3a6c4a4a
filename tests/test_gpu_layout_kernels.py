"""The layout kernels the engine selects by batch size and shape, against exact answers (C ABI, no solve):
  * ce_transpose (k_transpose<64>; k_transpose<32> in a child process started with CE_TR_TILE=32, which is read once per process): bit-exact
    against numpy's transpose at shapes that fill, overfill and underfill a tile on either side;
  * ce_parammap_apply2 on every branch of its selection (k_parammap<1> below B = 1024, k_parammap<4> from B = 1024, k_parammap_lds when B >= 256
    and cols * 8 <= 64 KiB; accumulate 0 / 1): against an exact sum of the products (math.fsum) within k 2^-53 sum |terms| for a row of k entries;
    rows around the 2048-row pass of k_parammap_lds, empty rows, groups of four rows that mix single- and multi-entry rows, padded leading dimensions;
    rows without entries are 0 (accumulate = 0) whatever the parameters are -- also +-Inf / NaN -- and bit-untouched (accumulate = 1);
  * ce_status_summary: min / counts of a status vector (negative codes, adjoint bit fields) against numpy, through pinned and pageable host memory."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from cvxpylayers_amd import _lib
from cvxpylayers_amd import problems as P

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U53 = 2.0 ** -53


def _engine():
    from cvxpylayers_amd.interfaces.mi355_if import ConeEngine
    tpl = P.dense_template(3, {"z": 0, "l": 4, "q": []})
    return ConeEngine(tpl.indices, tpl.indptr, tpl.n, tpl.m, tpl.cones, torch.device("cuda", 0))


# ------------------------------------------------------------------------------------------------ transpose
TRANSPOSE_SHAPES = [(1, 1), (1, 257), (257, 1), (1, 64), (64, 1)] + [(r, c) for r in (63, 64, 65) for c in (63, 64, 65)] + \
                   [(31, 33), (32, 32), (4096, 111), (111, 4097)]


def check_transposes():
    eng = _engine()
    rng = np.random.default_rng(0)
    L = _lib.lib()
    for rows, cols in TRANSPOSE_SHAPES:
        a = rng.standard_normal((rows, cols))
        src = torch.from_numpy(a).cuda()
        out = torch.full((cols * rows + 64,), float("nan"), dtype=torch.float64, device="cuda")      # (+64: a write past the result shows up as a changed sentinel)
        _lib.check(L.ce_transpose(eng._h, rows, cols, src.data_ptr(), out.data_ptr(), eng._stream()), "ce_transpose")
        got = out.cpu().numpy()
        assert np.array_equal(got[:rows * cols].reshape(cols, rows), a.T), (rows, cols)
        assert np.isnan(got[rows * cols:]).all(), (rows, cols)
    return len(TRANSPOSE_SHAPES)


def test_transpose_tile64_bit_exact():
    assert check_transposes() == len(TRANSPOSE_SHAPES)


def test_transpose_tile32_bit_exact_in_a_child_process():
    env = dict(os.environ, CE_TR_TILE="32", PYTHONPATH=os.pathsep.join([HERE, ROOT, os.environ.get("PYTHONPATH", "")]))
    code = "import test_gpu_layout_kernels as t; print('transposed', t.check_transposes())"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"transposed {len(TRANSPOSE_SHAPES)}" in r.stdout


# ------------------------------------------------------------------------------------------------ parameter maps
def make_map(rows, cols, seed):
    """CSR (rows x cols).  Rows r with r % 512 < 192 hold 0 or 1 entry (so that many of k_parammap_lds's groups of four rows r, r + 512, r + 1024, r + 1536
    take its one-entry branch, empty rows included); the others 0, 1, 2, 3 or 5 entries (groups that mix both kinds).  Columns 0 and cols - 1 are used."""
    rng = np.random.default_rng(seed)
    r = np.arange(rows)
    cnt = np.where(r % 512 < 192, rng.integers(0, 2, rows), rng.choice([0, 1, 2, 3, 5], rows))
    cnt[0] = max(cnt[0], 1)
    if rows > 1:
        cnt[-1] = max(cnt[-1], 1)
    indptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    nnz = int(indptr[-1])
    indices = rng.integers(0, cols, nnz).astype(np.int32)
    indices[0] = cols - 1
    indices[-1] = 0
    vals = rng.standard_normal(nnz) * np.exp2(rng.integers(-20, 20, nnz))
    return indptr, indices, vals


def run_map(B, rows, cols, acc, indptr, indices, vals, Pm, ld_out, out0):
    """ce_parammap_apply2 on device copies; Pm (B, ld_p) host; out0 (B, ld_out) host initial contents.  Returns the result on the host."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_ptr, d_idx, d_val, d_P, d_out = t(indptr), t(indices), t(vals), t(Pm), t(out0)
    rc = _lib.lib().ce_parammap_apply2(0, B, rows, cols, int(acc), d_ptr.data_ptr(), d_idx.data_ptr(), d_val.data_ptr(), d_P.data_ptr(), Pm.shape[1],
                                       d_out.data_ptr(), ld_out, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "ce_parammap_apply2")
    return d_out.cpu().numpy()


def two_product(a, b):
    """a * b = p + e exactly (Dekker / Veltkamp splitting; no overflow at the magnitudes used here)"""
    p = a * b
    sa = 134217729.0 * a; ah = sa - (sa - a); al = a - ah
    sb = 134217729.0 * b; bh = sb - (sb - b); bl = b - bh
    return [p, ((ah * bh - p) + ah * bl + al * bh) + al * bl]


def exact_check(got, base, acc, indptr, indices, vals, Pm, rows, fsum_rows_of):
    """got (B, >= rows): the map's result (+ base when acc) within k 2^-53 sum |terms| of the exact value.  The reference is a long-double sum for every
    instance (64-bit mantissa: its own error is covered by the 2^-64 term of the bound), and math.fsum of the exact products for the instances in
    fsum_rows_of."""
    B = got.shape[0]
    cnt = np.diff(indptr)
    has = cnt > 0
    row_of = np.repeat(np.arange(rows), cnt)
    terms = vals[None, :] * Pm[:, indices]                              # (rounded products: only for the bound)
    absum = np.zeros((B, rows)); np.add.at(absum.T, row_of, np.abs(terms).T)
    ld = vals[None, :].astype(np.longdouble) * Pm[:, indices].astype(np.longdouble)
    ref = np.zeros((B, rows), dtype=np.longdouble); np.add.at(ref.T, row_of, ld.T)
    if acc:
        ref = ref + base[:, :rows].astype(np.longdouble)
        absum = absum + np.abs(base[:, :rows])
    k = np.maximum(cnt, 1)[None, :] + (1 if acc else 0)
    bound = (1.001 * k * U53 + 64 * 2.0 ** -64 * k) * absum
    err = np.abs(got[:, :rows].astype(np.longdouble) - ref).astype(np.float64)
    sel = np.broadcast_to(has[None, :], err.shape)
    assert (err[sel] <= bound[sel]).all(), float((err - bound)[sel].max())
    for b in fsum_rows_of:
        for r in np.flatnonzero(has):
            t0, t1 = indptr[r], indptr[r + 1]
            parts = [base[b, r]] if acc else []
            for v, p in zip(vals[t0:t1], Pm[b, indices[t0:t1]]):
                parts += two_product(float(v), float(p))
            ex = math.fsum(parts)                                       # exact products, exact sum rounded once
            assert abs(got[b, r] - ex) <= bound[b, r] + U53 * abs(ex), (b, r, got[b, r], ex)
    # rows without entries: 0 (accumulate = 0), the initial contents bit for bit (accumulate = 1)
    if acc:
        assert np.array_equal(got[:, :rows][:, ~has].view(np.int64), base[:, :rows][:, ~has].view(np.int64))
    else:
        assert (got[:, :rows][:, ~has] == 0).all()


SENTINEL = np.frombuffer(np.array([0x7ff8dead0000beef], dtype=np.uint64).tobytes(), dtype=np.float64)[0]      # a NaN with a payload of its own


def kernel_for(B, cols):
    if cols > 0 and cols * 8 <= 64 * 1024 and B >= 256:
        return "lds"
    return "nb4" if B >= 1024 else "nb1"


@pytest.mark.parametrize("cols", [8192, 8193])
@pytest.mark.parametrize("B", [1, 255, 256, 1023, 1024, 1029])
def test_parammap_every_selection_branch(B, cols):
    rows = 2049
    indptr, indices, vals = make_map(rows, cols, seed=B * 7 + cols)
    rng = np.random.default_rng(B + cols)
    ld_p, ld_out = cols + 3, rows + 5                                   # padded leading dimensions on both sides
    Pm = rng.standard_normal((B, ld_p)) * np.exp2(rng.integers(-8, 8, (B, ld_p)))
    Pm[:, cols:] = np.nan                                               # the padding of a source row must never be read
    for acc in (0, 1):
        base = rng.standard_normal((B, ld_out)) if acc else np.full((B, ld_out), SENTINEL)
        base[:, rows:] = SENTINEL
        empty = np.flatnonzero(np.diff(indptr) == 0)
        if acc:
            base[:, empty[: len(empty) // 2]] = SENTINEL                # accumulate: empty rows keep whatever they hold, NaN payloads included
        got = run_map(B, rows, cols, acc, indptr, indices, vals, Pm, ld_out, base)
        assert np.array_equal(got[:, rows:].view(np.int64), base[:, rows:].view(np.int64)), "write past the row / into the padding"
        exact_check(got, base, acc, indptr, indices, vals, Pm, rows, fsum_rows_of=sorted({0, B // 2, B - 1}))
    print(f"B={B} cols={cols}: {kernel_for(B, cols)}")


@pytest.mark.parametrize("rows", [1, 511, 512, 513, 2047, 2048, 2049, 4097])
def test_parammap_lds_row_passes(rows):
    """k_parammap_lds walks the rows in passes of U * 512 = 2048 (four rows per thread): rows that end inside, at and just past a pass."""
    B, cols = 256, 300
    indptr, indices, vals = make_map(rows, cols, seed=rows)
    rng = np.random.default_rng(rows)
    Pm = rng.standard_normal((B, cols))
    for acc in (0, 1):
        base = rng.standard_normal((B, rows + 1)) if acc else np.full((B, rows + 1), SENTINEL)
        got = run_map(B, rows, cols, acc, indptr, indices, vals, Pm, rows + 1, base)
        assert np.array_equal(got[:, rows:].view(np.int64), base[:, rows:].view(np.int64))
        exact_check(got, base, acc, indptr, indices, vals, Pm, rows, fsum_rows_of=[0, B - 1])


@pytest.mark.parametrize("B,cols", [(1, 64), (300, 64), (1100, 9000), (300, 9000), (1100, 64)])
def test_parammap_empty_rows_are_zero_for_non_finite_parameters(B, cols):
    """The sum over no entries is 0 (include/cone_engine.h ce_parammap_apply) on all three kernels, also when the instance's parameter 0 -- the column an
    empty row of k_parammap_lds's one-entry branch used to multiply by 0.0 -- is +-Inf or NaN."""
    rows = 2048
    indptr, indices, vals = make_map(rows, cols, seed=3)
    rng = np.random.default_rng(4)
    Pm = rng.standard_normal((B, cols))
    Pm[:, 0] = np.array([np.inf, -np.inf, np.nan])[np.arange(B) % 3]
    cnt = np.diff(indptr)
    empty = cnt == 0
    uses0 = np.zeros(rows, dtype=bool)
    uses0[np.repeat(np.arange(rows), cnt)[indices == 0]] = True
    got = run_map(B, rows, cols, 0, indptr, indices, vals, Pm, rows, np.full((B, rows), SENTINEL))
    assert (got[:, empty] == 0).all(), f"{kernel_for(B, cols)}: {np.isnan(got[:, empty]).sum()} empty rows are not 0"
    clean = ~uses0
    exact_check(got[:, clean], None, 0, np.concatenate([[0], np.cumsum(cnt[clean])]).astype(np.int32),
                np.concatenate([indices[indptr[r]:indptr[r + 1]] for r in np.flatnonzero(clean)] + [np.zeros(0, np.int32)]),
                np.concatenate([vals[indptr[r]:indptr[r + 1]] for r in np.flatnonzero(clean)] + [np.zeros(0)]), Pm, int(clean.sum()), fsum_rows_of=[0])


def test_parammap_apply_without_cols():
    """ce_parammap_apply (no column count: never the LDS kernel) at both batch-size branches."""
    L = _lib.lib()
    rows, cols = 700, 50
    indptr, indices, vals = make_map(rows, cols, seed=9)
    for B in (1023, 1024):
        Pm = np.random.default_rng(B).standard_normal((B, cols))
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        d = [t(indptr), t(indices), t(vals), t(Pm), t(np.full((B, rows), SENTINEL))]
        _lib.check(L.ce_parammap_apply(0, B, rows, *(x.data_ptr() for x in d[:4]), cols, d[4].data_ptr(), rows,
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), "ce_parammap_apply")
        exact_check(d[4].cpu().numpy(), None, 0, indptr, indices, vals, Pm, rows, fsum_rows_of=[0, B - 1])


# ------------------------------------------------------------------------------------------------ status summary
@pytest.mark.parametrize("B", [1, 63, 64, 255, 256, 257, 100000])
def test_status_summary_against_numpy(B):
    eng = _engine()
    L = _lib.lib()
    rng = np.random.default_rng(B)
    codes = np.array([1, 2, -1, -2, -4, -6, -7, 0, 4, 8, 12, 3, 5, 9, 15])      # solver statuses and adjoint bit fields
    pinned = torch.zeros(4, dtype=torch.int32).pin_memory()          # (one buffer for the engine's lifetime: ce_status_summary remembers its device alias)
    pageable = np.zeros(4, dtype=np.int32)
    for trial in range(3):
        v = rng.choice(codes, B).astype(np.int32)
        if trial == 1:
            v[:] = 1
        if trial == 2:
            v[-1] = -7                                                   # the minimum in the last element (the tail of the last wave)
        d = torch.from_numpy(v).cuda()
        want = [int(v.min()), int((v == 2).sum()), int(((v & 3) != 0).sum()), 1]
        for host in (pinned.data_ptr(), pageable.ctypes.data):
            _lib.check(L.ce_status_summary(eng._h, B, d.data_ptr(), host, eng._stream()), "ce_status_summary")
            torch.cuda.synchronize()
        assert pinned.tolist() == want, (B, trial, pinned.tolist(), want)
        assert pageable.tolist() == want, (B, trial, pageable.tolist(), want)
