"""Writes tests/golden/plan_table.json: the launch plan (csrc/ce_plan.h, compiled with g++) over the grid of plan_kit.plan_grid().

The committed table was recorded from the commit BEFORE the plan became a host unit (the same shim around that commit's cone_engine.hip, passed here as a shared
object), so tests/test_plan_host.py pins the host unit to what ce_create planned then.  Re-record it, without an argument, only with a change that is meant to move
a plan: a new row of ce_variants.h, a changed footprint.

    python tests/golden/make_plan_table.py [shim.so]
"""
import ctypes
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import plan_kit as pk          # noqa: E402

if __name__ == "__main__":
    results = pk.run_grid(pk.plan_grid(), lib=ctypes.CDLL(sys.argv[1]) if len(sys.argv) > 1 else None)
    out = os.path.join(HERE, "plan_table.json")
    with open(out, "w") as f:
        f.write(json.dumps(pk.encode_table(results), separators=(",", ":")).replace("]],", "]],\n"))
    print(f"{len(results)} calls -> {out} ({os.path.getsize(out)} bytes)")
