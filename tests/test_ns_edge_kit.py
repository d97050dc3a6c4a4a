"""The inputs of tests/test_gpu_ns_mode_edges.py, proven without a GPU: edge discovery over the three planners of k_backward_ns on the g++ build of the plan
(plan_kit.NS_FAMILIES), and every planted instance (ns_edge_kit.plant) of every shape the GPU test uses -- both sides of every edge that are served, and the
structure shapes -- is a regular KKT point: J finite, cond(J) <= 1e11, KKT residual <= 1e-13 (1 + max(|b|, |c|)).  No instance is left out on the reference's
account.  Also: the union member each union shape was made for is the largest one, the three states of a triple occur, and the host shim is clean under
-fsanitize=address,undefined as a stand-alone program."""
import subprocess

import numpy as np
import pytest

import ns_edge_kit as K
import plan_kit as pk


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for e in pk.PLAN_ENV:
        monkeypatch.delenv(e, raising=False)


def test_edges_of_the_three_planners_are_found():
    table = K.edge_table()
    print("\nedges of the three planners (family: value before | after, kind's row before -> after, resolve_fits before -> after):")
    for fam, kind, vb, pb, va, pa in table:
        f = pk.NS_KIND_FIELD[kind]
        row = lambda p: -1 if p is None else p[f]          # noqa: E731
        fit = lambda p: None if p is None else p["resolve_fits"]          # noqa: E731
        lds = lambda p: None if p is None else p[f.replace("variant", "lds")]          # noqa: E731
        print(f"  {fam}: {vb} | {va}  row {row(pb)} -> {row(pa)}  resolve_fits {fit(pb)} -> {fit(pa)}  lds {lds(pb)} -> {lds(pa)}")
    by_fam = {}
    for fam, kind, vb, pb, va, pa in table:
        by_fam.setdefault(fam, []).append((pb, pa))
    # every family ends in a refusal (ns_family_values runs until then), and the n sweeps change row before it
    for fam, (kind, _, _) in pk.NS_FAMILIES.items():
        assert by_fam[fam][-1][1] is None, fam
        rows = [pb[pk.NS_KIND_FIELD[kind]] for pb, _ in by_fam[fam]]
        assert rows == sorted(rows), (fam, rows)
    for kind in pk.NS_KIND_FIELD:
        reached = {pb[pk.NS_KIND_FIELD[kind]] for fam, k, _, pb, _, _ in table if k == kind}
        assert reached == {r[0] for r in pk.variant_rows("CE_NS_VARIANTS")}, (kind, reached)
    # a served plan serves its own kind alone
    for name, (shape, plan, what) in K.edge_cases().items():
        if plan is not None:
            assert sum(plan[f] >= 0 for f in pk.NS_FIELDS) == 1, (name, plan)
    resolve = [(fam, vb, va) for fam, kind, vb, pb, va, pa in table if pb is not None and pa is not None and pb["resolve_fits"] != pa["resolve_fits"]]
    print("  resolve_lds_fits edges with the kind still served:", resolve or "none")


def test_union_shapes_make_their_member_the_largest():
    for name, member in K.UNION_LARGEST.items():
        for kind, shape in K.STRUCTURE[name].items():
            plan = pk.host_ns_plan(shape)
            row = plan[pk.NS_KIND_FIELD[kind]]
            n, cones = shape[1], shape[2]
            abc = pk.ns_union_members(n, K.P.cone_rows(cones), len(cones["q"]), row)
            print(name, kind, "row", row, "a, b, c =", abc)
            assert abc[member] == max(abc) and sorted(abc)[-1] > sorted(abc)[-2], (name, kind, abc)
    # the rows of the m = 400 shape outnumber the threads of its row, and its cone lies behind row 256
    shape = K.STRUCTURE["union_c_n4_m400"]["plain"]
    assert pk.variant_rows("CE_NS_VARIANTS")[pk.host_ns_plan(shape)["ns_variant"]][2] == 256 and shape[2]["z"] + shape[2]["l"] > 256


# the edge shapes are discovered, so the cases are grouped by what is known at collection: a family of plan_kit.NS_FAMILIES, or a structure shape and its kind
GROUPS = list(pk.NS_FAMILIES) + [f"{name}:{kind}" for name, by in K.STRUCTURE.items() for kind in by]


@pytest.mark.parametrize("group", GROUPS)
def test_every_planted_instance_is_a_regular_kkt_point(group):
    cases = K.cases_of(group)
    assert any(what != "refused" for _, _, what in cases.values()), group
    for name, (shape, plan, what) in cases.items():
        if what == "refused":
            continue
        pt = K.point(name, shape, **K.plant_args(name))
        cond, resid = K.regularity(pt)
        print(f"\n{name}: n {pt['n']} m {pt['m']} B {cond.size} k1 {pt['k1'].min()}..{pt['k1'].max()} nf {pt['nf'].min()}..{pt['nf'].max()} "
              f"cond max {cond.max():.2e} KKT residual max {resid.max():.2e}")
        assert np.isfinite(cond).all() and (cond <= 1e11).all(), (name, cond)
        assert (resid <= 1e-13).all(), (name, resid)
        assert (pt["k1"] <= pt["n"]).all() and (pt["kind"] == "qp" or (pt["k1"] + pt["L"] >= pt["n"]).all()), name
        if shape[0] != "qp" and pt["L"].min() > 0 and (pt["k1"] - pt["nf"] < pt["n"]).all():
            assert pt["nf"].min() > 0, (name, "the reduced Hessian is empty")


def test_the_two_dense_references_are_transposes_of_each_other():
    """the references of tests/test_gpu_ns_many_edges.py against each other, at every served plain and qp case: the oracle's dense adjoint (with P for the QP kind)
    at that file's first cotangent draw and dense_jvp at tangents(pt) satisfy
        <xb, dx> + <yb, dy> = <dA, tA> + <db, tb> + <dc, tc> (+ <dP, tP>)
    within 1e-10 (1 + |lhs| + |rhs|) on every instance -- dense symmetric dP against dense symmetric tP.  Both are backward-stable dense solves of systems with
    cond <= 1e11 whose right-hand sides are O(1): the identity's two sides differ by eps cond |solution|^2 at the very worst, and by far less in practice."""
    from oracle import oracle
    worst = ("", 0.0)
    for name, (shape, plan, what) in K.all_cases().items():
        kind = shape[0]
        if kind == "tri" or not pk.ns_served(kind, plan):
            continue
        pt = K.point(name, shape, **K.plant_args(name))
        rng = np.random.default_rng(pt["seed"] + 31)
        xb, yb = rng.standard_normal(pt["x"].shape), rng.standard_normal(pt["y"].shape)
        kw = dict(P=pt["Pm"]) if kind == "qp" else {}
        g = oracle.adjoint_batch(pt["A"], pt["b"], pt["c"], pt["cones"], pt["x"], pt["y"], pt["s"], xb, yb, mode="dense", **kw)
        tA, tb, tc, tP = t = K.tangents(pt)
        dx, dy, ds, ok = K.dense_jvp(pt, t)
        assert ok.all(), (name, ok)
        lhs = (xb * dx).sum(axis=1) + (yb * dy).sum(axis=1)
        rhs = (g["dA"] * tA).sum(axis=(1, 2)) + (g["db"] * tb).sum(axis=1) + (g["dc"] * tc).sum(axis=1)
        if kind == "qp":
            assert np.abs(g["dP"] - g["dP"].transpose(0, 2, 1)).max() <= 1e-12 * (1 + np.abs(g["dP"]).max()), name          # the dense dP is symmetric
            rhs = rhs + (g["dP"] * tP).sum(axis=(1, 2))
        e = np.abs(lhs - rhs) / (1 + np.abs(lhs) + np.abs(rhs))
        print(f"{name}: transpose identity of the two references max {e.max():.2e}, max |lhs| {np.abs(lhs).max():.2e}")
        assert (e <= 1e-10).all() and np.abs(lhs).max() > 1e-3, (name, e)
        worst = max(worst, (name, float(e.max())), key=lambda w: w[1])
    print("worst:", worst)


def test_the_three_states_of_a_triple_occur():
    seen = np.zeros(3, int)
    for name, (shape, plan, what) in K.all_cases().items():
        if shape[0] == "tri" and what != "refused":
            seen += K.point(name, shape, **K.plant_args(name))["triple_states"]
    print("triples with D = I, D = 0, on the boundary:", seen)
    assert (seen > 0).all(), seen


def test_host_shim_is_clean_under_the_sanitizers(tmp_path):
    """the stand-alone walker of tests/plan_host.cpp (its own main) built with -fsanitize=address,undefined, with the planners' entry called on every edge shape"""
    src = tmp_path / "ns_walk.cpp"
    calls = []
    for name, (shape, plan, what) in K.edge_cases().items():
        kind, n, cones, _ = shape
        calls.append(f"  {{ int q[] = {{{', '.join(str(d) for d in cones['q']) or '0'}}}; double p[] = {{{', '.join(str(a) for a in cones.get('p', [])) or '0'}}}; "
                     f"one({n}, {cones['z']}, {cones['l']}, {len(cones['q'])}, q, {cones.get('ep', 0)}, {len(cones.get('p', []))}, p, {int(kind == 'qp')}); }}")
    src.write_text('#include "' + str(pk.ROOT) + '/tests/plan_host.cpp"\n' + r'''
static void one(int n, int z, int l, int nq, int *q, int ep, int np_, double *p, int qp) {
    int m = z + l + 3 * ep + 3 * np_;
    for (int k = 0; k < nq; k++) m += q[k];
    std::vector<int> indices, indptr(1, 0), pidx, pptr(1, 0);
    for (int j = 0; j <= n; j++) { for (int i = 0; i < m; i++) indices.push_back(i); indptr.push_back((int)indices.size()); }
    for (int j = 0; qp && j < n; j++) { for (int i = 0; i <= j; i++) pidx.push_back(i); pptr.push_back((int)pidx.size()); }
    ce_template t{};
    t.n = n; t.m = m; t.nnz_aug = (int)indices.size(); t.indices = indices.data(); t.indptr = indptr.data(); t.z = z; t.l = l; t.nq = nq; t.q = q; t.nep = ep; t.np = np_; t.p = p;
    if (qp) { t.nnz_p = (int)pidx.size(); t.p_indices = pidx.data(); t.p_indptr = pptr.data(); }
    long out[8]; const int rc = h_plan_ns(&t, out);
    printf("%d", rc); for (int i = 0; rc == 0 && i < 7; i++) printf(" %ld", out[i]); printf("\n");
    for (int v = 0; v < 3; v++) { long u[6]; h_ns_union(n, m, nq, v, u); }
}
int main() {
''' + "\n".join(calls) + "\n  return 0;\n}\n")
    exe = tmp_path / "ns_walk"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__host__=", "-D__device__=",
                           f"-DN_PLAN_FIELDS={len(pk.PLAN_FIELDS)}", "-I", f"{pk.ROOT}/cvxpylayers_amd/csrc", "-I", f"{pk.ROOT}/include", "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    cases = list(K.edge_cases().values())
    assert len(lines) == len(cases)
    for line, (shape, plan, what) in zip(lines, cases):          # the program and the shared object plan alike
        host = pk.host_ns_plan(shape)
        got = [int(t) for t in line.split()]
        assert got == ([0] + [host[f] for f in pk.NS_PLAN_FIELDS] if host is not None else got[:1]) and (host is not None or got[0] != 0), (shape, got, host)
