"""Host side of the many-cotangent adjoint and the many-tangent forward derivative for templates with PSD blocks (no device): ce_vjp_psd_many, ce_jvp_psd_many and
their two variant queries are declared, bound and exported under the unchanged ABI version, refuse bad arguments before any device call, and solver_args
psd_adjoint / psd_tangents take their two values and no third.

The modes add no layout mode and no row: they run on the footprint of the blocks' forward modes (psd_ns_variant, psd_ns_lds), and each is an object of its own, not a
mode of csrc/ce_tu_ns.hip or csrc/ce_tu_ns_psd.hip.  Their argument structs are named NsVjpManyPsd and NsJvpManyPsd, NOT Ns...Many: the ledger of
tests/test_gpu_ns_many_edges.py collects the ce_launch_ns overloads of ce_types.h whose type matches Ns\\w*Many and requires exactly the five modes that file covers;
these modes' edge ledger is tests/test_gpu_psd_many_edges.py.  All of that is pinned here."""
import ctypes as C
import os
import re

import pytest

from cvxpylayers_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ce_vjp_psd_many", "ce_vjp_psd_many_variant", "ce_jvp_psd_many", "ce_jvp_psd_many_variant")


def test_entry_points_are_declared_bound_and_exported():
    """fails on a tree without the modes: the symbols are absent"""
    hdr = open(os.path.join(ROOT, "include", "cone_engine.h")).read()
    for name in ("ce_vjp_psd_many", "ce_jvp_psd_many"):
        assert re.search(rf"\bint {name}\(ce_handle h, int B, int K,", hdr) and re.search(rf"\bint {name}_variant\(ce_handle h\);", hdr), name
    assert "ce_vjp_psd_many, ce_jvp_psd_many, ce_vjp_psd_many_variant and ce_jvp_psd_many_variant" in hdr          # (named in the ABI history under 17)
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.SYMBOLS and getattr(L, name) is not None
    assert len(L.ce_vjp_psd_many.argtypes) == 17 and L.ce_vjp_psd_many.argtypes == L.ce_vjp_many.argtypes          # (arguments and layouts are ce_vjp_many's)
    assert len(L.ce_jvp_psd_many.argtypes) == 27 and L.ce_jvp_psd_many.argtypes == L.ce_jvp_many.argtypes          # (and ce_jvp_many's)
    assert len(L.ce_vjp_psd_many_variant.argtypes) == 1 and len(L.ce_jvp_psd_many_variant.argtypes) == 1
    assert L.ce_vjp_psd_many_variant(None) == -1 and L.ce_jvp_psd_many_variant(None) == -1


def test_abi_version_and_plan_fields_are_unchanged():
    from cvxpylayers_amd.interfaces import cone_engine as CEI
    hdr = open(os.path.join(ROOT, "include", "cone_engine.h")).read()
    assert int(re.search(r"#define CE_ABI_VERSION (\d+)", hdr).group(1)) == 17 == _lib.lib().ce_abi_version() == _lib.ABI_VERSION
    fields = CEI.ConeEngine.PLAN_FIELDS
    assert len(fields) == 18 and not any("psd" in f for f in fields), fields


def _vjp(L, h, B, K, p, **null):
    a = dict(A=p, x=p, y=p, s=p, dx=p, dy=p, dA=p, dq=p, adj=p)
    a.update(null)
    return L.ce_vjp_psd_many(h, B, K, a["A"], 1, None, 0, 0, a["x"], a["y"], a["s"], a["dx"], a["dy"], a["dA"], a["dq"], a["adj"], None)


def _jvp(L, h, B, K, p, stA_b=0, stq_b=0, **null):
    a = dict(A=p, x=p, y=p, s=p, tA=p, tq=p, dx=p, dy=p, ds=p, st=p, it=p)
    a.update(null)
    return L.ce_jvp_psd_many(h, B, K, a["A"], 1, None, 0, 0, a["x"], a["y"], a["s"], a["tA"], 1, stA_b, a["tq"], 1, stq_b, a["dx"], a["dy"], a["ds"], a["st"], a["it"],
                             1e-8, 1e-8, 1e8, 0, None)


def test_bad_arguments_are_refused_before_any_device_call():
    L = _lib.lib()
    buf = (C.c_double * 8)()
    p = C.addressof(buf)
    # K <= 0, B <= 0, a null required pointer, a negative batch stride: refused on the arguments alone (the handle is never looked at: a block of zeros stands for it)
    fake = (C.c_char * 4096)()
    h = C.addressof(fake)
    for call, who, required in ((_vjp, b"ce_vjp_psd_many", ("A", "x", "y", "s", "dx", "dA", "dq")), (_jvp, b"ce_jvp_psd_many", ("A", "x", "y", "s", "dx", "dy", "st"))):
        assert call(L, None, 1, 1, p) == -1 and who in L.ce_last_error()          # CE_E_BADARG: null handle
        assert call(L, h, 1, 0, p) == -1 and call(L, h, 1, -3, p) == -1 and call(L, h, 0, 2, p) == -1 and call(L, h, -1, 2, p) == -1
        assert who in L.ce_last_error()
        for name in required:
            assert call(L, h, 1, 2, p, **{name: None}) == -1, (who, name)
        assert who in L.ce_last_error()
    assert _jvp(L, h, 1, 2, p, stA_b=-1) == -1 and _jvp(L, h, 1, 2, p, stq_b=-1) == -1
    assert b"ce_jvp_psd_many" in L.ce_last_error()


def test_the_two_keys_take_their_two_values_and_no_third():
    from cvxpylayers_amd.interfaces import solver_args as SA
    assert "psd_adjoint" in SA._KNOWN_ARGS and "psd_tangents" in SA._KNOWN_ARGS
    assert SA.psd_adjoint({}) == "pivoting" and SA.psd_adjoint({"psd_adjoint": "pivoting"}) == "pivoting" and SA.psd_adjoint({"psd_adjoint": "search_free"}) == "search_free"
    assert SA.psd_tangents({}) == "loop" and SA.psd_tangents({"psd_tangents": "loop"}) == "loop" and SA.psd_tangents({"psd_tangents": "many"}) == "many"
    for bad in ("Search_free", "", None, 1, "many", "off"):
        with pytest.raises(ValueError, match="psd_adjoint"):
            SA.psd_adjoint({"psd_adjoint": bad})
    for bad in ("Many", "", None, 1, "search_free", "off"):
        with pytest.raises(ValueError, match="psd_tangents"):
            SA.psd_tangents({"psd_tangents": bad})
    # the keys are independent of psd_elimination, whose values and default stay
    assert SA.psd_elimination({"psd_adjoint": "search_free", "psd_tangents": "many"}) == "off"
    assert SA.psd_adjoint({"psd_elimination": "search_free"}) == "pivoting" and SA.psd_tangents({"psd_elimination": "search_free"}) == "loop"


def test_an_unserved_template_gets_one_notice_per_key_and_a_template_without_blocks_none():
    import warnings
    from cvxpylayers_amd.interfaces import solver_args as SA
    for key in ("psd_adjoint", "psd_tangents"):
        SA._WARNED.discard(key + "_none")
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            assert SA.psd_many_active(key, True, 2, True) is True and SA.psd_many_active(key, False, 2, True) is False
            assert SA.psd_many_active(key, True, -1, False) is False and SA.psd_many_active(key, False, -1, True) is False
            assert not w, [str(x.message) for x in w]
            assert SA.psd_many_active(key, True, -1, True) is False and SA.psd_many_active(key, True, -1, True) is False
        assert len(w) == 1 and key in str(w[0].message), [str(x.message) for x in w]


def test_the_objects_and_the_untouched_mode_lists():
    csrc = os.path.join(ROOT, "cvxpylayers_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    objs = mk.split("OBJS")[1].split("all:")[0]
    for unit, obj in (("ce_tu_ns_vjp_psd_many.hip", "$(OBJDIR)/ns_vjp_psd_many.o"), ("ce_tu_ns_jvp_psd_many.hip", "$(OBJDIR)/ns_jvp_psd_many.o")):
        assert unit in mk and obj in objs and os.path.exists(os.path.join(csrc, unit)), unit
        src = open(os.path.join(csrc, unit)).read()
        assert "CE_NS_VARIANTS(X)" in src and src.count("true, true>") == 2, unit          # every row, launch and attribute alike: <..., MANY = true, PSD = true>
    src = open(os.path.join(csrc, "ce_tu_ns.hip")).read()
    lists = re.findall(r"#define NS_MODES\(Y\)(.*)", src)
    modes = [m for line in lists for m in re.findall(r"Y\((?:true|false), (?:true|false), (?:true|false), (?:true|false), (\w+)\)", line)]
    assert len(lists) == 3 and len(modes) == 7 and not any("Psd" in m for m in modes), modes
    psd = open(os.path.join(csrc, "ce_tu_ns_psd.hip")).read()
    assert psd.count("k_backward_ns<NTILE") == 2 and psd.count("k_backward_ns<NTILE, NTHR, true, REF, false, false, false, true>") == 2          # (x 3 rows x REF or not: its six)
    for setter in ("ce_setattr_ns_vjp_psd_many", "ce_setattr_ns_jvp_psd_many"):
        assert setter in open(os.path.join(csrc, "ce_types.h")).read() and setter in open(os.path.join(csrc, "cone_engine.hip")).read()


def test_the_ledger_of_the_many_modes_keeps_its_five_names_and_these_modes_have_their_own():
    """the regular expression is the one tests/test_gpu_ns_many_edges.py::test_ledger_of_rows_and_many_modes parses ce_types.h with"""
    types = open(os.path.join(ROOT, "cvxpylayers_amd", "csrc", "ce_types.h")).read()
    names = re.findall(r"int ce_launch_ns\([^;]*const (Ns\w*Many) &w\);", types)
    assert sorted(names) == ["NsJvpMany", "NsJvpQpMany", "NsMany", "NsVjpQpMany", "NsVjpTriMany"], names
    for name, base in (("NsVjpManyPsd", "NsMany"), ("NsJvpManyPsd", "NsJvpMany")):
        assert not re.fullmatch(r"Ns\w*Many", name)
        assert re.search(rf"int ce_launch_ns\([^;]*const {name} &w\);", types) and re.search(rf"struct {name} : {base} \{{\}};", types), name
    edges = open(os.path.join(ROOT, "tests", "test_gpu_psd_many_edges.py")).read()
    assert "ce_vjp_psd_many" in edges and "ce_jvp_psd_many" in edges and "def test_every_row_is_reached_by_a_compared_call_of_each_mode" in edges
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "NsVjpManyPsd" in design and "NsJvpManyPsd" in design and "3.19" in design
