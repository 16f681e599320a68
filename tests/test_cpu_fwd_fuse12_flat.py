"""The two C-ABI symbols of the fused conv1 -> conv2 forward (xt_net_set_fwd_fuse12_flat, xt_conv12_valid_fwd): the header,
the ctypes table of xingtian_amd/lib.py and the built library agree on them, argument by argument."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _want(header, name, structs):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
    assert m, name
    ctype_of = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    want = []
    for arg in m.group(1).split(","):
        words = arg.replace("*", " * ").split()
        if "*" in words:
            pointee = [w for w in words if w not in ("const", "*")][0]
            want.append(structs.get(pointee, ctypes.c_void_p))
        else:
            want.append(ctype_of[[w for w in words if w != "const"][0]])
    return want


def test_header_ctypes_table_and_library_agree_on_the_new_symbols():
    from xingtian_amd import lib
    header = open(os.path.join(ROOT, "include", "xt_mi355x.h")).read()
    structs = {"xt_conv_geom": ctypes.POINTER(lib.ConvGeom), "xt_input_xform": ctypes.POINTER(lib.InputXform)}
    handle = lib.load()
    for name in ("xt_net_set_fwd_fuse12_flat", "xt_conv12_valid_fwd"):
        assert name in lib.SIGNATURES and hasattr(handle, name), name
        res, args = lib.SIGNATURES[name]
        want = _want(header, name, structs)
        assert res is ctypes.c_int32 and len(args) == len(want), (name, len(args), len(want))
        for i, (a, w) in enumerate(zip(args, want)):
            assert a is w, (name, i, a, w)
    assert lib.SIGNATURES["xt_net_set_fwd_fuse12_flat"] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32])
    assert len(lib.SIGNATURES["xt_conv12_valid_fwd"][1]) == 15


def test_the_switch_is_per_net_and_on_by_default():
    """neither a tuning knob nor a step-report word was added; the Python wrapper mirrors the library's default"""
    from xingtian_amd import lib
    from xingtian_amd.model.hip_net import HipActorCritic
    assert "fwd_fuse12_flat" not in [n for n, _ in lib.Tuning._fields_]
    assert len(lib.Tuning._fields_) == 34 and len(lib.STEP_REPORT_NET) == 12 and len(lib.STEP_REPORT_LAYER) == 8
    assert HipActorCritic.fwd_fuse12_flat_on is True and callable(HipActorCritic.set_fwd_fuse12_flat)
