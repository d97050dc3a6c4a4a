"""The launch plan is a host unit (cvxpylayers_amd/csrc/ce_plan.h: no HIP call, no HIP include), so it is checked here without a GPU, compiled with g++ behind the
shim tests/plan_host.cpp:
  * against the commit before it became one: tests/golden/plan_table.json holds what that commit's plan_engine, pack_rows, sa_fwd_select and sa_lsqr_select returned
    (recorded through the same shim around its cone_engine.hip, tests/golden/make_plan_table.py) over plan_kit.plan_grid() -- every value of every family under
    every create-time switch, and both shared-A selectors over the cone sets, call kinds and call-time switches of test_gpu_plan_edges.py.  The table keeps the
    plans as runs (plan_kit.encode_table): every plan of the grid must have its run's fields, and the sizes (LDS bytes among them) the recorded ones at both
    ends of every run, where a plan changes; every other call is kept whole.  The host build must reproduce every number;
  * the create-time half of that test's coverage ledger: its discovery, run through the host plan, reaches every entry of EXPECTED that a plan alone reaches (all but
    the rows of the shared-A kernels' lists, which count only through a compared call) with the same EXPECTED_UNREACHABLE;
  * memory safety: a stand-alone program (its own main, nothing loaded into python) built with -fsanitize=address,undefined walks the same grid through plan_engine,
    pack_rows and the selectors, exits 0 and prints the same numbers."""
import json
import os
import subprocess

import pytest

import plan_kit as pk

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plan_table.json")


@pytest.fixture(scope="module")
def grid():
    cmds = pk.plan_grid()
    return cmds, pk.run_grid(cmds)


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


def test_host_plan_reproduces_the_recorded_table(grid, recorded):
    _, results = grid
    n_plans = sum(len(list(pk.family_values(f))) for f in pk.all_families(ledger=True)) * len(pk.SWITCHES)
    assert sum(1 for key, _ in results if key[3] == "P") == n_plans
    diffs = pk.table_differences(results, recorded)
    print(f"\n{len(results)} calls compared ({n_plans} plans), {len(diffs)} differences")
    assert not diffs, diffs[:10]


def test_ledger_create_time_half(monkeypatch):
    import test_gpu_plan_edges as edges          # (its discovery and ledger names; importing it needs no GPU)
    assert edges.SWITCHES == pk.SWITCHES
    monkeypatch.setattr(edges, "_CACHE", {})
    monkeypatch.setattr(pk, "plan_of", lambda fam, v, device=None: pk.host_plan_of(fam, v))
    for e in pk.PLAN_ENV:
        monkeypatch.delenv(e, raising=False)
    shapes, seen, kept = edges.discovery()
    assert not [(fam, v) for fam, v, p in seen.values() if p["fwd_mode"] == 4 and not p["aa_ok"]]
    ledger = {var for fam, v, p in seen.values() for var in edges.variants_of(p, fam)}
    for sw in edges.SWITCHES[1:]:
        with monkeypatch.context() as mp:
            for e, val in sw.items():
                mp.setenv(e, val)
            ledger |= {var for fam, vals in shapes.items() for v in vals for p in [pk.host_plan_of(fam, v)] if p is not None for var in edges.variants_of(p, fam)}
    by_call_only = {edges.sa_fwd_name(*r[1:]) for r in pk.variant_rows("CE_SA_FWD_VARIANTS")} | {edges.sa_lsqr_name(*r[1:]) for r in pk.variant_rows("CE_SA_LSQR_VARIANTS")}
    missing = [var for var in edges.EXPECTED if var not in by_call_only and var not in ledger and var not in edges.EXPECTED_UNREACHABLE]
    assert not missing, missing
    assert not [var for var in edges.EXPECTED_UNREACHABLE if var in ledger], "an entry listed as unreachable was reached"


def test_host_unit_under_sanitizers(tmp_path, grid, recorded):
    cmds, results = grid
    exe = pk.host_build(tmp_path, program=True, extra=["-g", "-fsanitize=address,undefined", "-static-libasan", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"])
    pk.write_grid(cmds, tmp_path / "grid.txt")
    env = {k: v for k, v in os.environ.items() if k not in pk.PLAN_ENV}
    run = subprocess.run([exe, str(tmp_path / "grid.txt")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env)
    assert run.returncode == 0, run.stderr[-4000:]
    lines = [tuple(int(x) for x in ln.split()) for ln in run.stdout.splitlines()]
    assert len(lines) == len(results)
    diffs = pk.table_differences([(key, got) for (key, _), got in zip(results, lines)], recorded)
    assert not diffs, diffs[:10]
