"""The inputs of tests/test_gpu_psd_mode_edges.py, proven without a GPU: edge discovery over the two PSD-bearing planners of k_backward_ns on the g++ build of the
plan (psd_edge_kit.FAMILIES), each refusal attributed to its gate; every planted instance (psd_edge_kit.plant) of every shape the GPU test compares is a regular KKT
point -- J finite, cond(J) <= 1e11, KKT residual <= 1e-13 (1 + max(|b|, |c|)), every weighted PSD row and every triple's interior eigenvalue at least
100 x NS_TRI_STIFF from 0 and 1 -- so that no instance is left out of a reference and the stiff rule flags none; the dense adjoint and the dense forward solve are
transposes of each other; the comparison the GPU test applies rejects a reference with one B_ab off by 1e-4 and one with two rows of a block's Q swapped; and the
host shim is clean under -fsanitize=address,undefined as a stand-alone program."""
import subprocess

import numpy as np
import pytest

import plan_kit as pk
import psd_edge_kit as K
import psd_ns_kit as PK


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for e in pk.PLAN_ENV:
        monkeypatch.delenv(e, raising=False)


def test_edges_of_the_two_planners_are_found_and_attributed():
    table = K.edge_table()
    print("\nedges of the PSD-bearing planners (family:kind: value before | after, row before -> after, the gate that refuses the far side):")
    for fam, kind, vb, rb, va, ra, gate in table:
        print(f"  {fam}:{kind}: {vb} | {va}  row {rb} -> {ra}" + (f"  refused by {gate}" if gate else ""))
    rows = {r[0] for r in pk.variant_rows("CE_NS_VARIANTS")}
    for fam, (kinds, _, fn) in K.FAMILIES.items():
        for kind in kinds:
            mine = [e for e in table if e[:2] == (fam, kind)]
            assert mine and mine[-1][5] == -1 and mine[-1][6] in K.GATES, (fam, kind, mine)          # every family ends in a refusal with a gate to its name
            assert [e[3] for e in mine] == sorted(e[3] for e in mine), (fam, kind, mine)
    for kind in K.KIND_FIELDS:
        assert {e[3] for e in table if e[1] == kind} == rows, kind          # the n sweep reaches every row
        gates = {e[6] for e in table if e[1] == kind and e[6]}
        print(f"  gates met by the {kind} kind: {sorted(gates)}")
        assert {"footprint", "resolve"} <= gates, (kind, gates)          # both gates of the plan, beside the column rule
    # the shim's two gates compose to the plan's answer at every case, and a served shape serves its own kind alone
    for name, (shape, row, gate) in K.all_cases().items():
        g = K.gates(shape)
        assert g is not None, name
        want = g["first_fit"] if g["resolve_fits"] else -1
        vf, lf = K.KIND_FIELDS[shape[0]]
        other = K.KIND_FIELDS["mixed" if shape[0] == "psd" else "psd"][0]
        assert g[vf] == want == row and g[other] == -1, (name, g, row)
        assert (g[lf] == g["first_fit_lds"] == K.host_plan(shape)["lds"]) if row >= 0 else gate in K.GATES, (name, g)
        assert gate != "footprint" or not g["footprint_fits"] or not g["columns_fit"], (name, g)


def test_structure_shapes_are_on_their_rows_and_are_what_they_are_named_for():
    rows = pk.variant_rows("CE_NS_VARIANTS")
    for name, row in K.STRUCTURE_ROW.items():
        for kind, shape in K.STRUCTURE[name].items():
            assert K.host_plan(shape)["variant"] == row, (name, kind, K.host_plan(shape))
    for r in range(3):
        for kind, shape in K.STRUCTURE[f"blocks_over_waves_row{r}"].items():
            assert len(shape[2]["s"]) == rows[r][2] // 64 + 1
    for kind, shape in K.STRUCTURE["psd_rows_over_threads"].items():
        assert K.TK.psd_rows(shape[2]) > rows[0][2] > shape[2]["s"][0] * (shape[2]["s"][0] + 1) // 2
    for kind, shape in K.STRUCTURE["all_in"].items():
        assert shape[4] == tuple(shape[2]["s"])
    for kind, shape in K.STRUCTURE["all_out_z_is_n"].items():
        assert set(shape[4]) == {0} and shape[2]["z"] == shape[1]


@pytest.mark.parametrize("group", K.GROUPS)
def test_every_planted_instance_is_a_regular_kkt_point(group):
    cases = K.cases_of(group)
    assert any(row >= 0 for _, row, _ in cases.values()), group
    stiff = K.stiff_constant()
    for name, (shape, row, gate) in cases.items():
        if row < 0:
            continue
        pt = K.case_point(name)
        cond, resid = K.regularity(pt)
        bm, tm = K.margins(pt)
        print(f"\n{name}: n {pt['n']} m {pt['m']} B {cond.size} row {row} k1 {pt['k1'].min()}..{pt['k1'].max()} L {pt['L'].min()}..{pt['L'].max()} nf {pt['nf'].min()}..{pt['nf'].max()} "
              f"cond max {cond.max():.2e} KKT residual max {resid.max():.2e} smallest min(B, 1 - B) {bm:.3f} smallest triple margin {tm:.3f} "
              f"reference uncertainty {K.reference_uncertainty(pt):.1e} median bound {K.median_bound(pt):.1e}")
        assert np.isfinite(cond).all() and (cond <= 1e11).all(), (name, cond)
        assert (resid <= 1e-13).all(), (name, resid)
        assert bm >= 100 * stiff and tm >= 100 * stiff, (name, bm, tm)
        assert (pt["k1"] <= pt["n"]).all() and (pt["k1"] + pt["L"] >= pt["n"]).all(), name
        # the planted decomposition and numpy's agree on what is weighted: p (k - p) rows per block
        for i in range(cond.size):
            for (r0, k), p in zip(PK.blocks({**pt["cones"], "ep": 0, "p": []}), shape[4]):
                Bv = PK.block_eig(pt["v"][i, r0:r0 + k * (k + 1) // 2], k)[3]
                assert int(((Bv != 0.0) & (Bv != 1.0)).sum()) == p * (k - p) and int((Bv == 1.0).sum()) == p * (p + 1) // 2, (name, i, k, p)
        # nothing is filtered: both references and the Newton step exist on every instance (the >= 80 % share of the GPU test is the siblings' cap, not a filter)
        assert K.median_bound(pt) == 1e-8, (name, K.reference_uncertainty(pt))
        x1, y1, s1, v1 = K.perturbed(pt)
        assert K.dense_newton(pt, x1, v1)[2].all(), name


def test_the_two_dense_references_are_transposes_of_each_other():
    """psd_many_kit.dense_adjoint (with the mixed projection's D) at the GPU test's cotangent draws and psd_tri_ns_kit.dense_jvp at its tangent draws satisfy
        <xb, dx> + <yb, dy> = <dA, tA> + <db, tb> + <dc, tc>
    within 1e-10 (1 + |lhs| + |rhs|) on every instance of every compared shape (the bound of test_ns_edge_kit.py: two backward-stable dense solves of systems with
    cond <= 1e11 and O(1) right-hand sides)"""
    worst = ("", 0.0)
    for name, (shape, row, gate) in K.all_cases().items():
        if row < 0:
            continue
        pt = K.case_point(name)
        xb, yb = K.cotangents(pt)
        for d in (0, 1):
            g = K.want_adjoint(pt, d)
            tA, tb, tc = K.tangents(pt, d + 1)
            dx, dy, ds = K.want_forward(pt, d)
            lhs = (xb[d] * dx).sum(axis=1) + (yb[d] * dy).sum(axis=1)
            rhs = (g["dA"] * tA).sum(axis=(1, 2)) + (g["db"] * tb).sum(axis=1) + (g["dc"] * tc).sum(axis=1)
            e = np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))
            assert (e <= 1e-10).all() and np.abs(lhs).max() > 1e-3, (name, d, e)
            worst = max(worst, (name, float(e.max())), key=lambda w: w[1])
        print(f"{name}: transpose identity of the two references holds, max |lhs| {np.abs(lhs).max():.2e}")
    print("worst:", worst)


@pytest.mark.parametrize("name", ["n:psd[28]", "n:mixed[61]"])
def test_the_comparison_rejects_a_subtly_wrong_rotation(name, monkeypatch):
    """the yardstick of the GPU test (psd_edge_kit.hold with the shape's median bound) on a forward derivative computed with instance-independent mistakes in the
    first block: one weighted row's B_ab off by 1e-4, and two rows of the block's basis Q swapped.  It accepts the reference itself and rejects both."""
    pt = K.case_point(name)
    t = K.tangents(pt, 1)
    want = K.want_forward(pt, 0)
    reg = np.ones(pt["x"].shape[0], bool)
    med = K.median_bound(pt)
    K.hold(name, "the reference against itself", K.dense_jvp(pt, t)[:3], want, reg, med)
    k0 = pt["cones"]["s"][0]
    real = PK.block_eig

    def off_by(what):
        def block_eig(w, k):
            U, lam, Q, Bv = real(w, k)
            if k == k0 and what == "B":
                Bv = Bv.copy(); Bv[np.flatnonzero((Bv != 0.0) & (Bv != 1.0))[0]] += 1e-4
            if k == k0 and what == "Q":
                Q = Q.copy(); Q[[0, 1]] = Q[[1, 0]]
            return U, lam, Q, Bv
        return block_eig
    for what in ("B", "Q"):
        monkeypatch.setattr(PK, "block_eig", off_by(what))
        wrong = K.dense_jvp(pt, t)[:3]
        monkeypatch.setattr(PK, "block_eig", real)
        e = np.max([K.rel(g, w) for g, w in zip(wrong, want)], axis=0)
        with pytest.raises(AssertionError) as exc:
            K.hold(name, f"{what} wrong", wrong, want, reg, med)
        print(f"\n{name}: {'one B_ab + 1e-4' if what == 'B' else 'two rows of Q swapped'}: error max {e.max():.2e} median {np.median(e):.2e} -- rejected: {exc.value}")


def test_host_shim_is_clean_under_the_sanitizers(tmp_path):
    """a stand-alone program (its own main) around the shim of psd_edge_kit, built with -fsanitize=address,undefined, walks every case of the edge grid and the
    structure shapes; it plans as the shared object does"""
    cases = list(K.all_cases().values())
    arr = lambda xs, zero: ", ".join(str(x) for x in xs) or zero          # noqa: E731
    calls = []
    for shape, row, gate in cases:
        c = shape[2]
        calls.append(f"  {{ int q[] = {{{arr(c.get('q', []), '0')}}}; int s[] = {{{arr(c.get('s', []), '0')}}}; double p[] = {{{arr(c.get('p', []), '0')}}}; "
                     f"one({shape[1]}, {c.get('z', 0)}, {c.get('l', 0)}, {len(c.get('q', []))}, q, {len(c.get('s', []))}, s, {c.get('ep', 0)}, {len(c.get('p', []))}, p); }}")
    exe = K._compile(str(tmp_path / "psd_edge_walk"), K.HOST_SRC + K.HOST_MAIN + "int main() {\n" + "\n".join(calls) + "\n  return 0;\n}\n",
                     ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(cases)
    for line, (shape, row, gate) in zip(lines, cases):
        g = K.gates(shape)
        assert [int(t) for t in line.split()] == [0] + [g[f] for f in K.GATE_FIELDS], (shape, line, g)
