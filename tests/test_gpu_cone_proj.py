"""Pi_K of every cone kind, alone on the GPU (cvxpylayers_amd/cones.py project -> ce_cone_project): zero / nonnegative rows bit-equal to numpy's clip,
second-order cones against the closed form, PSD blocks against numpy.linalg.eigh, exponential / power triples against the oracle.  No instance is left out
of any comparison: the inputs are built away from kinks (cone_proj_kit.py), the deliberate kink points are tested against the stated convention."""
import numpy as np
import pytest
import torch

from cvxpylayers_amd import cones as CN, problems as P
from cvxpylayers_amd.interfaces.cone_set import ConeSet
import cone_proj_kit as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _proj(v, cones, dual=False):
    return CN.project(_t(v), cones, dual=dual).cpu().numpy()


def _soc_check(out, ref, v, cones):
    z, l = cones.get("z", 0), cones.get("l", 0)
    assert np.array_equal(out[:, :z + l], ref[:, :z + l])                                      # rows: bit-equal
    for a, b in K.soc_spans(cones):
        err = np.abs(out[:, a:b] - ref[:, a:b]).max(axis=1)
        assert (err <= 1e-13 * (1 + np.linalg.norm(v[:, a:b], axis=1))).all(), (b - a, err.max())


def _orth(out, v):
    """<Pi(v), Pi(v) - v> per instance, relative to ||v||^2"""
    return np.abs(np.sum(out * (out - v), axis=1)) / np.maximum(np.sum(v * v, axis=1), 1e-300)


@pytest.mark.parametrize("B", [1, 2, 65])
def test_rows_and_second_order_cones(B):
    rng = np.random.default_rng(B)
    v = K.rows_soc_input(rng, B)
    out = _proj(v, K.ROWS_SOC)
    _soc_check(out, K.rows_soc_ref(v), v, K.ROWS_SOC)
    assert (_orth(out, v) <= 2e-13).all()
    # the dual: the zero cone's dual is free, everything else is self-dual; and Moreau, Pi_K*(v) = v + Pi_K(-v)
    outd = _proj(v, K.ROWS_SOC, dual=True)
    _soc_check(outd, K.rows_soc_ref(v, dual=True), v, K.ROWS_SOC)
    moreau = v + _proj(-v, K.ROWS_SOC)
    for a, b in [(0, 5)] + K.soc_spans(K.ROWS_SOC):
        assert (np.abs(outd[:, a:b] - moreau[:, a:b]).max(axis=1) <= 1e-13 * (1 + np.linalg.norm(v[:, a:b], axis=1))).all()
    # a row pitch larger than m: the same bits
    m = v.shape[1]
    cs = ConeSet(K.ROWS_SOC, DEV)
    buf = torch.full((B, m + 3), 9.0, dtype=torch.float64, device=DEV)
    buf[:, :m] = _t(v)
    o2, st = cs.project(buf[:, :m], False, False)
    torch.cuda.synchronize()
    assert st is None and np.array_equal(o2.cpu().numpy(), out)


def test_second_order_cone_special_points():
    """the origin, z = 0 with either sign of t, and the exact boundary t = ||z|| (inclusive: the point itself) / t = -||z|| (0)"""
    cones = {"q": [5, 17]}
    v = np.zeros((5, 22))
    v[1, 0], v[1, 5] = -1.5, -0.25                           # z = 0, t < 0
    v[2, 0], v[2, 5] = 2.0, 0.75                             # z = 0, t > 0
    for i, sgn in ((3, 1.0), (4, -1.0)):                     # 3-4-5 triangles: ||z|| is exact
        v[i, 1:3] = (3.0, 4.0); v[i, 0] = sgn * 5.0
        v[i, 6:8] = (6.0, 8.0); v[i, 5] = sgn * 10.0
    out = _proj(v, cones)
    ref = K.rows_soc_ref(v, cones)
    assert np.array_equal(out[:3], ref[:3]) and np.array_equal(out[3], v[3]) and not out[4].any()


@pytest.mark.parametrize("orders", K.PSD_ORDERS, ids=lambda o: "s" + "_".join(map(str, o)))
@pytest.mark.parametrize("B", [1, 3])
def test_psd_blocks(orders, B):
    cones = {"s": orders}
    cs = ConeSet(cones, DEV)
    rng = np.random.default_rng(100 * B + orders[0])
    for kind in ("mixed", "positive", "negative", "zero", "rank_one", "repeated"):
        v, mats = K.psd_input(rng, B, orders, kind)
        out_t, state = cs.project(_t(v), False, True)
        out, state = out_t.cpu().numpy(), state.cpu().numpy()
        assert np.array_equal(_proj(v, cones), out)                                            # with and without the state: the same bits
        off = 0
        for S, X, k in zip(mats, K.psd_split(out, orders), orders):
            assert np.abs(X - K.psd_proj(S)).max() <= 3e-13 * max(np.abs(S).max(), 1.0), (k, kind)
            if kind == "positive":
                assert np.abs(X - S).max() <= 3e-13
            if kind in ("negative", "zero"):
                assert np.abs(X).max() <= 3e-13
            V = state[:, off:off + k * k].reshape(B, k, k); w = state[:, off + k * k:off + k * k + k]
            assert np.abs(V @ np.swapaxes(V, 1, 2) - np.eye(k)).max() <= 1e-11, (k, kind)
            assert np.abs(np.sort(w, axis=1) - np.linalg.eigvalsh(S)).max() <= 3e-13 * max(np.abs(S).max(), 1.0), (k, kind)      # the UNCLIPPED eigenvalues
            off += k * k + k
        assert (_orth(out, v) <= 2e-13).all(), kind
        assert np.array_equal(_proj(v, cones, dual=True), out)                                  # self-dual


def test_an_order_beyond_the_footprint_raises_and_launches_nothing():
    before = len(CN._SETS)
    with pytest.raises(NotImplementedError, match="largest supported order is 82"):
        CN.project(torch.zeros(2, 83 * 84 // 2, dtype=torch.float64, device=DEV), {"s": [83]})
    assert len(CN._SETS) == before                                                             # no handle exists: nothing could be launched
    k = 82                                                                                     # the largest supported order runs (the Jacobi path at its LDS bound)
    S = K.psd_matrices(np.random.default_rng(0), 1, k, "mixed")[0]
    X = P.svec_to_sym(_proj(P.sym_to_svec(S), {"s": [k]}), k)
    assert np.abs(X - K.psd_proj(S)).max() <= 3e-13 * max(np.abs(S).max(), 1.0)


def test_exponential_and_power_triples():
    """Projection within 1e-12 (1 + ||v||) of the oracle on 200 seeded points and within 1e-10 (1 + ||v||) on the special points (the tolerances of
    tests/test_expcone_host.py for the same routines on the host).  Orthogonality <Pi(v), Pi(v) - v> / ||v||^2: the oracle's own projection leaves at most
    2.9e-16 on these points (measured, and measured again here and printed); ten times what it leaves is allowed.  The device routine compiled for the host
    leaves 3.0e-16."""
    rng = np.random.default_rng(7)
    v = K.triple_points(rng, 200)
    spans = [(3 * c, 3 * c + 3) for c in range(4)]
    for dual in (False, True):
        out, ref = _proj(v, K.TRIPLES, dual=dual), K.triples_ref(v, dual=dual)
        worst, worst_ref = 0.0, 0.0
        for a, b in spans:
            err = np.abs(out[:, a:b] - ref[:, a:b]).max(axis=1)
            assert (err <= 1e-12 * (1 + np.linalg.norm(v[:, a:b], axis=1))).all(), (a, dual, err.max())
            worst = max(worst, _orth(out[:, a:b], v[:, a:b]).max()); worst_ref = max(worst_ref, _orth(ref[:, a:b], v[:, a:b]).max())
        print(f"triples dual={dual}: orthogonality residual {worst:.3e}, the oracle's own {worst_ref:.3e}")
        assert worst <= 10 * worst_ref
    sp = np.tile(np.asarray(K.SPECIAL_TRIPLES), (1, 4))
    for dual in (False, True):
        out, ref = _proj(sp, K.TRIPLES, dual=dual), K.triples_ref(sp, dual=dual)
        assert np.isfinite(out).all()
        for a, b in spans:
            assert (np.abs(out[:, a:b] - ref[:, a:b]).max(axis=1) <= 1e-10 * (1 + np.linalg.norm(sp[:, a:b], axis=1))).all(), (a, dual)


ALL = {"z": 2, "l": 3, "q": K.Q_DIMS, "s": [3, 17, 40], "ep": 2, "p": [0.3, -0.6]}


def _all_kinds_input(rng, B):
    parts = [K.rows_soc_input(rng, B), K.psd_input(rng, B, ALL["s"], "mixed")[0], K.triple_points(rng, B)]
    return parts, np.concatenate(parts, axis=1)


def test_all_kinds_in_one_set_equal_the_per_kind_results_bit_for_bit():
    parts, v = _all_kinds_input(np.random.default_rng(3), 65)
    for dual in (False, True):
        out = _proj(v, ALL, dual=dual)
        per_kind = np.concatenate([_proj(parts[0], K.ROWS_SOC, dual), _proj(parts[1], {"s": ALL["s"]}, dual), _proj(parts[2], K.TRIPLES, dual)], axis=1)
        assert np.array_equal(out, per_kind)
    mod = CN.ConeProjection(ALL).to(DEV)
    assert np.array_equal(mod(_t(v).reshape(5, 13, -1)).cpu().numpy().reshape(65, -1), _proj(v, ALL)) and len(mod._sets) == 1


def test_a_nan_stays_inside_the_cone_that_holds_it():
    """(the host harness of tests/test_cone_proj_host.py runs the triple routine on the same non-finite inputs first)"""
    parts, v = _all_kinds_input(np.random.default_rng(4), 5)
    clean = _proj(v, ALL)
    assert np.isfinite(clean).all()
    m0 = parts[0].shape[1]; s0 = m0 + 6; e0 = m0 + parts[1].shape[1]
    soc = K.soc_spans(ALL)[4]                                  # the cone of dimension 17
    psd = (s0, s0 + 17 * 18 // 2)                              # the block of order 17
    tri = (e0 + 6, e0 + 9)                                     # the first power cone
    v[2, tri[0]:tri[1]] = (0.5, 1.0, 1.0)
    clean = _proj(v, ALL)
    bad = v.copy()
    bad[2, soc[0] + 9] = np.nan; bad[2, psd[0] + 40] = np.nan; bad[2, tri[0]] = np.nan          # the triple is the harness's [nan, 1, 1], then [inf, 1, 1]
    out = _proj(bad, ALL)
    mask = np.zeros_like(v, dtype=bool)
    for a, b in (soc, psd, tri):
        mask[2, a:b] = True
    assert np.isnan(out[mask]).all()                           # exactly those cones ...
    assert np.array_equal(out[~mask], clean[~mask])            # ... and every other row of the batch bit-equal to the run without it
    out = _proj(np.where(np.isnan(bad), np.inf, bad), ALL)     # the same with an infinity
    assert np.isnan(out[mask]).all() and np.array_equal(out[~mask], clean[~mask])
    z = _proj(np.array([[np.nan, 1.0, -np.inf, np.nan]]), {"z": 2, "l": 2})
    assert np.isnan(z[0, 0]) and z[0, 1] == 0.0 and z[0, 2] == 0.0 and np.isnan(z[0, 3])


def test_dtype_and_device_of_the_result_follow_the_input():
    v = torch.randn(4, 2, 8, device=DEV, dtype=torch.float32)
    out = CN.project(v, {"l": 3, "q": [5]})
    assert out.dtype == torch.float32 and out.device == v.device and out.shape == v.shape
    ref = K.rows_soc_ref(v.double().cpu().numpy().reshape(8, 8), {"l": 3, "q": [5]})
    assert np.abs(out.double().cpu().numpy().reshape(8, 8) - ref).max() <= 1e-6
    X = torch.randn(3, 4, 4, device=DEV, dtype=torch.float64)
    Y = CN.project_psd(X)
    S = 0.5 * (X + X.transpose(1, 2)).cpu().numpy()
    assert np.abs(Y.cpu().numpy() - K.psd_proj(S)).max() <= 3e-13 * max(np.abs(S).max(), 1.0) and torch.equal(Y, Y.transpose(1, 2))
