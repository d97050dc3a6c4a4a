"""Host side of the many-cotangent adjoint for templates with exponential / power triples (no device): ce_vjp_tri_many and ce_vjp_tri_many_variant are declared,
bound and exported under the unchanged ABI version, refuse bad arguments before any device call, and solver_args tri_adjoint takes its two values and no third.

The mode adds no layout mode and no row: it runs on the footprint of the triples' forward modes (ce_ns_layout.h, ce_plan.h and CE_NS_VARIANTS are untouched; the
plan table and tests/test_ns_layout_host.py pin them), and it is an object of its own, not a mode of csrc/ce_tu_ns.hip: the three NS_MODES lists there keep their
seven entries (tests/test_gpu_ns_mode_edges.py builds its ledger from them; this mode's ledger is tests/test_gpu_vjp_tri_many_edges.py)."""
import ctypes as C
import os
import re

import pytest

from cvxpylayers_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ce_vjp_tri_many", "ce_vjp_tri_many_variant")


def test_entry_points_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "cone_engine.h")).read()
    assert re.search(r"\bint ce_vjp_tri_many\(ce_handle h, int B, int K,", hdr) and re.search(r"\bint ce_vjp_tri_many_variant\(ce_handle h\);", hdr)
    assert "ce_vjp_tri_many and ce_vjp_tri_many_variant" in hdr          # (named in the ABI history under 17)
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
    assert len(L.ce_vjp_tri_many.argtypes) == 17 and len(L.ce_vjp_tri_many_variant.argtypes) == 1
    assert L.ce_vjp_tri_many.argtypes == L.ce_vjp_many.argtypes          # (arguments and layouts are ce_vjp_many's)
    assert L.ce_vjp_tri_many_variant(None) == -1


def test_abi_version_stays_17():
    hdr = open(os.path.join(ROOT, "include", "cone_engine.h")).read()
    assert int(re.search(r"#define CE_ABI_VERSION (\d+)", hdr).group(1)) == 17 == _lib.lib().ce_abi_version() == _lib.ABI_VERSION


def _call(L, h, B, K, p, **null):
    a = dict(A=p, q=p, x=p, y=p, s=p, dx=p, dy=p, dA=p, dq=p, st=p)
    a.update(null)
    return L.ce_vjp_tri_many(h, B, K, a["A"], 1, a["q"], 1, 1, a["x"], a["y"], a["s"], a["dx"], a["dy"], a["dA"], a["dq"], a["st"], None)


def test_bad_arguments_are_refused_before_any_device_call():
    L = _lib.lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    assert _call(L, None, 1, 1, p) == -1 and b"ce_vjp_tri_many" in L.ce_last_error()          # CE_E_BADARG: null handle
    # K <= 0, B <= 0, a null required pointer: refused on the arguments alone (the handle is never looked at: a block of zeros stands for it)
    fake = (C.c_char * 4096)()
    h = C.addressof(fake)
    assert _call(L, h, 1, 0, p) == -1 and _call(L, h, 1, -3, p) == -1 and _call(L, h, 0, 2, p) == -1 and _call(L, h, -1, 2, p) == -1
    assert b"ce_vjp_tri_many" in L.ce_last_error()
    for name in ("A", "x", "y", "s", "dx", "dA", "dq"):
        assert _call(L, h, 1, 2, p, **{name: None}) == -1, name


def test_tri_adjoint_takes_its_two_values_and_no_third():
    from cvxpylayers_amd.interfaces import solver_args as SA
    assert "tri_adjoint" in SA._KNOWN_ARGS
    assert SA.tri_adjoint({}) == "pivoting" and SA.tri_adjoint({"tri_adjoint": "pivoting"}) == "pivoting" and SA.tri_adjoint({"tri_adjoint": "search_free"}) == "search_free"
    for bad in ("searchfree", "", None, 1, "Pivoting"):
        with pytest.raises(ValueError, match="tri_adjoint"):
            SA.tri_adjoint({"tri_adjoint": bad})


def test_the_mode_lists_of_the_single_right_hand_side_object_are_unchanged_in_number():
    src = open(os.path.join(ROOT, "cvxpylayers_amd", "csrc", "ce_tu_ns.hip")).read()
    lists = re.findall(r"#define NS_MODES\(Y\)(.*)", src)
    modes = [m for line in lists for m in re.findall(r"Y\((?:true|false), (?:true|false), (?:true|false), (?:true|false), (\w+)\)", line)]
    assert len(lists) == 3 and len(modes) == 7 and "NsVjpTriMany" not in modes, modes
    mk = open(os.path.join(ROOT, "cvxpylayers_amd", "csrc", "Makefile")).read()
    assert "ce_tu_ns_vjp_tri_many.hip" in mk and "$(OBJDIR)/ns_vjp_tri_many.o" in mk.split("OBJS")[1].split("all:")[0]
