"""Host side of the many-tangent forward derivative for templates with exponential / power triples (no device): ce_jvp_tri_many and ce_jvp_tri_many_variant are
declared, bound and exported under the unchanged ABI version, refuse bad arguments before any device call, and solver_args tri_tangents takes its two values and no
third.

The mode adds no layout mode and no row: it runs on the footprint of the triples' forward modes, and it is an object of its own, not a mode of csrc/ce_tu_ns.hip:
the three NS_MODES lists there keep their seven entries.  Its argument struct is named NsJvpManyTri, NOT Ns...Many: the ledger of tests/test_gpu_ns_many_edges.py
collects the ce_launch_ns overloads of ce_types.h whose type matches Ns\\w*Many and requires exactly the five modes that file covers; this mode's edge ledger is
tests/test_gpu_jvp_tri_many_edges.py.  Both facts are pinned here."""
import ctypes as C
import os
import re

import pytest

from cvxpylayers_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ce_jvp_tri_many", "ce_jvp_tri_many_variant")


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cone_engine.h")).read()
    assert re.search(r"\bint ce_jvp_tri_many\(ce_handle h, int B, int K,", hdr) and re.search(r"\bint ce_jvp_tri_many_variant\(ce_handle h\);", hdr)
    assert "ce_jvp_tri_many and ce_jvp_tri_many_variant" in hdr          # (named in the ABI history under 17)
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
    assert len(L.ce_jvp_tri_many.argtypes) == 27 and len(L.ce_jvp_tri_many_variant.argtypes) == 1
    assert L.ce_jvp_tri_many.argtypes == L.ce_jvp_many.argtypes          # (arguments and layouts are ce_jvp_many's)
    assert L.ce_jvp_tri_many_variant(None) == -1


def test_abi_version_stays_17():
    hdr = open(os.path.join(ROOT, "include", "cone_engine.h")).read()
    assert int(re.search(r"#define CE_ABI_VERSION (\d+)", hdr).group(1)) == 17 == _lib.lib().ce_abi_version() == _lib.ABI_VERSION


def _call(L, h, B, K, p, stA_b=0, stq_b=0, **null):
    a = dict(A=p, x=p, y=p, s=p, tA=p, tq=p, dx=p, dy=p, ds=p, st=p, it=p)
    a.update(null)
    return L.ce_jvp_tri_many(h, B, K, a["A"], 1, None, 0, 0, a["x"], a["y"], a["s"], a["tA"], 1, stA_b, a["tq"], 1, stq_b, a["dx"], a["dy"], a["ds"], a["st"], a["it"],
                             1e-8, 1e-8, 1e8, 0, None)


def test_bad_arguments_are_refused_before_any_device_call():
    L = _lib.lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    assert _call(L, None, 1, 1, p) == -1 and b"ce_jvp_tri_many" in L.ce_last_error()          # CE_E_BADARG: null handle
    # K <= 0, B <= 0, a null required pointer, a negative batch stride: refused on the arguments alone (the handle is never looked at: a block of zeros stands for it)
    fake = (C.c_char * 4096)()
    h = C.addressof(fake)
    assert _call(L, h, 1, 0, p) == -1 and _call(L, h, 1, -3, p) == -1 and _call(L, h, 0, 2, p) == -1 and _call(L, h, -1, 2, p) == -1
    assert b"ce_jvp_tri_many" in L.ce_last_error()
    for name in ("A", "x", "y", "s", "dx", "dy", "st"):
        assert _call(L, h, 1, 2, p, **{name: None}) == -1, name
    assert _call(L, h, 1, 2, p, stA_b=-1) == -1 and _call(L, h, 1, 2, p, stq_b=-1) == -1
    assert b"ce_jvp_tri_many" in L.ce_last_error()


def test_tri_tangents_takes_its_two_values_and_no_third():
    from cvxpylayers_amd.interfaces import solver_args as SA
    assert "tri_tangents" in SA._KNOWN_ARGS
    assert SA.tri_tangents({}) == "loop" and SA.tri_tangents({"tri_tangents": "loop"}) == "loop" and SA.tri_tangents({"tri_tangents": "many"}) == "many"
    for bad in ("Many", "", None, 1, "search_free"):
        with pytest.raises(ValueError, match="tri_tangents"):
            SA.tri_tangents({"tri_tangents": bad})


def test_the_mode_lists_of_the_single_right_hand_side_object_are_unchanged_in_number():
    src = open(os.path.join(ROOT, "cvxpylayers_amd", "csrc", "ce_tu_ns.hip")).read()
    lists = re.findall(r"#define NS_MODES\(Y\)(.*)", src)
    modes = [m for line in lists for m in re.findall(r"Y\((?:true|false), (?:true|false), (?:true|false), (?:true|false), (\w+)\)", line)]
    assert len(lists) == 3 and len(modes) == 7 and "NsJvpManyTri" not in modes, modes
    mk = open(os.path.join(ROOT, "cvxpylayers_amd", "csrc", "Makefile")).read()
    assert "ce_tu_ns_jvp_tri_many.hip" in mk and "$(OBJDIR)/ns_jvp_tri_many.o" in mk.split("OBJS")[1].split("all:")[0]


def test_the_ledger_of_the_many_modes_keeps_its_five_names_and_this_mode_has_its_own():
    """the regular expression is the one tests/test_gpu_ns_many_edges.py::test_ledger_of_rows_and_many_modes parses ce_types.h with"""
    types = open(os.path.join(ROOT, "cvxpylayers_amd", "csrc", "ce_types.h")).read()
    names = re.findall(r"int ce_launch_ns\([^;]*const (Ns\w*Many) &w\);", types)
    assert sorted(names) == ["NsJvpMany", "NsJvpQpMany", "NsMany", "NsVjpQpMany", "NsVjpTriMany"], names
    assert re.search(r"int ce_launch_ns\([^;]*const NsJvpManyTri &w\);", types) and re.search(r"struct NsJvpManyTri : NsJvpMany \{\};", types)
    edges = open(os.path.join(ROOT, "tests", "test_gpu_jvp_tri_many_edges.py")).read()
    assert "NsJvpManyTri" in edges and "ce_jvp_tri_many" in edges and "def test_every_row_is_reached_by_a_compared_call" in edges
    assert "NsJvpManyTri" in open(os.path.join(ROOT, "DESIGN.md")).read()          # (where the name is explained beside the declaration's comment)
