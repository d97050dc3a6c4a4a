"""The many-cotangent adjoint and the many-tangent forward derivative with PSD blocks (ce_vjp_psd_many / NsVjpManyPsd, ce_jvp_psd_many / NsJvpManyPsd) at the edges
of their launch plan: psd_ns_kit's shapes reach rows 0 and 2 of CE_NS_VARIANTS only, so four edge shapes (psd_many_kit.EDGES, B = 8) straddle the column limits of
the rows -- 4 ceil(n / 4) + 1 <= 32 at n = 28 (row 0) and not at n = 29 (row 1), <= 64 at n = 60 (row 1) and not at n = 61 (row 2).  Both modes at K = 3 against the
dense references of psd_many_kit, with the tolerances of test_gpu_vjp_psd_many.py / test_gpu_jvp_psd_many.py (1e-5 worst, 1e-8 median relative to
1 + max |reference| on status-0 instances, >= 80 %).  Every instance is Solved by the oracle, the dense systems have condition numbers <= 1.4e3, and the smallest
min(B, 1 - B) of a weighted row is 3.0e-3 (checked on the CPU): nothing is filtered, nothing is flagged by the stiff rule.

Ledger: every row of CE_NS_VARIANTS (parsed from ce_variants.h) must be reached by a compared call of each mode.  The footprint edges, n = 108 and the structure
shapes are in tests/test_gpu_psd_mode_edges.py."""
import pytest

import plan_kit as pk
import psd_many_kit as M
import psd_ns_kit as K
from cvxpylayers_amd import _lib

pytestmark = pytest.mark.gpu
KC = 3
_REACHED: dict = {"ce_vjp_psd_many": {}, "ce_jvp_psd_many": {}}


def _row(name):
    r = M.point(name, n_draws=1)
    L = _lib.lib()
    want = K.host_plan(*M.EDGES[name][:2])["psd_ns_variant"]
    assert want == M.EDGES[name][4], (name, want)
    assert L.ce_vjp_psd_many_variant(r["eng"]._h) == L.ce_jvp_psd_many_variant(r["eng"]._h) == L.ce_psd_ns_variant(r["eng"]._h) == want
    return r, want


def _run(name, mode):
    if name in _REACHED[mode]:
        return
    r, row = _row(name)
    (M.check_vjp_against_dense if mode == "ce_vjp_psd_many" else M.check_jvp_against_dense)(r, KC)
    _REACHED[mode][name] = row          # (only a call that was compared counts)


@pytest.mark.parametrize("name", list(M.EDGES))
def test_many_cotangents_at_the_edge(name):
    _run(name, "ce_vjp_psd_many")


@pytest.mark.parametrize("name", list(M.EDGES))
def test_many_tangents_at_the_edge(name):
    _run(name, "ce_jvp_psd_many")


def test_every_row_is_reached_by_a_compared_call_of_each_mode():
    rows = [r[0] for r in pk.variant_rows("CE_NS_VARIANTS")]
    assert rows == [0, 1, 2], rows
    for mode in _REACHED:
        for name in M.EDGES:
            _run(name, mode)
        got = {row: [n for n, r in _REACHED[mode].items() if r == row] for row in rows}
        print(f"ledger of {mode}: " + ", ".join(f"row {row}: {got[row]}" for row in rows))
        assert all(got[row] for row in rows), (mode, got)
