"""CPU checks that the case table of tests/test_gpu_gauss_heads.py covers ppo_gauss_heads_fused_kernel: every
NQ x PART x SHARED instance has a case, the parameter values and both sides of every threshold are there, the float64
reference of every case, re-run here, leaves no row within the margin of a branch boundary and populates all four gradient
outcomes; the header, the ctypes prototypes and xt_tuning are in step; the geometries the kernel refuses are refused before
any device call.  An instance added without a case fails here, on any box."""
import ctypes
import importlib.util
import itertools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    """the GPU module imported for its table and its numpy references only (no test of it runs)"""
    tests = os.path.join(ROOT, "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)          # (it imports its helpers from test_gpu_heads_branch.py)
    spec = importlib.util.spec_from_file_location("_gauss_heads_cases", os.path.join(tests, "test_gpu_gauss_heads.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_gauss_head_instance_has_a_case(cases):
    G = cases.GAUSS_CASES
    ids = [c.id for c in G]
    assert len(ids) == len(set(ids))
    # nq_of and the instance list restate the dispatch of launch_ppo_gauss_heads_fused (csrc/xt_heads.hip)
    nq_of = lambda f: 1 if f <= 64 else 2 if f <= 128 else 4 if f <= 256 else 8
    for c in G:
        assert c.nq == nq_of(c.F) and c.B <= 40 and c.A <= 8 and c.F <= 512, c.id
    for nq, part, shared in itertools.product((1, 2, 4, 8), (False, True), (False, True)):
        assert [c for c in G if (c.nq, bool(c.ks), c.shared) == (nq, part, shared)], \
            "ppo_gauss_heads_fused_kernel<{}, {}, {}>: no case".format(nq, part, shared)


def test_gauss_cases_hold_the_parameter_values_and_both_sides_of_every_threshold(cases):
    G = cases.GAUSS_CASES
    assert {c.F for c in G} == {1, 37, 64, 65, 100, 128, 200, 256, 300, 512}        # 64|65, 128|200, 256|300 by NQ
    assert {c.A for c in G} == {1, 3, 6, 8} and {c.B for c in G} == {1, 3, 40}
    assert {2, 3, 5, 16} <= {k for c in G if c.ks for k in c.ks}
    assert any(c.ks and not c.shared and c.ks[0] != c.ks[1] for c in G)
    for sel in (lambda c: not c.ks, lambda c: bool(c.ks)):
        assert {"relu", "tanh"} <= {c.act for c in G if sel(c)}
    assert any(c.idx for c in G) and any(not c.idx for c in G) and cases.POOL_EXTRA == 13
    assert sum(c.inv_b_mul == 0.5 for c in G) == 1 and all(c.inv_b_mul in (0.5, 1.0) for c in G)
    assert any(c.stats for c in G) and any(not c.stats for c in G)
    assert (cases.CLIP, cases.ENT, cases.VF_CLIP, cases.CRITIC, cases.MARGIN) == (0.1, 0.003, 0.5, 0.7, 1e-4)


def test_gauss_references_leave_no_row_near_a_boundary_and_populate_every_gradient_branch(cases):
    big = 0
    for c in cases.GAUSS_CASES:
        d = cases.gauss_data(c)
        ref = cases.gauss_reference(c, d)
        keep = ref["keep"]
        assert keep.all(), (c.id, int((~keep).sum()))
        for k in ("mean", "value", "dmean", "dvalue", "dls_rows", "terms"):
            assert np.isfinite(ref[k]).all(), (c.id, k)
        assert d["action"].dtype == np.float32 and d["action"].shape == (c.B + cases.POOL_EXTRA, c.A), c.id
        if c.idx:
            assert len(set(d["idx"].tolist())) == c.B and d["idx"].max() >= c.B, c.id
        if c.B == 40:
            big += 1
            assert set(ref["pops"]) == {"dsurr_adv", "dsurr_zero", "dv_live", "dv_zero"}
            for k, v in ref["pops"].items():
                assert v >= 0.10, (c.id, k, v)
    assert big >= 8


def test_header_prototypes_and_tuning_are_in_step(cases):
    from xingtian_amd import lib
    header = open(os.path.join(ROOT, "include", "xt_mi355x.h")).read()
    assert cases.gauss_family() == 4 == lib.HEAD_PATH_PPO_GAUSS_FUSED
    assert cases.gauss_family() not in cases.HB.head_paths().values()
    for name in ("xt_net_set_gauss_fused", "xt_ppo_gauss_heads_fused_ex"):
        assert name in lib.SIGNATURES and hasattr(lib.load(), name), name
    assert lib.SIGNATURES["xt_net_set_gauss_fused"] == (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_int32])
    # the stand-alone entry against its declaration, argument by argument
    m = re.search(r"\bint\s+xt_ppo_gauss_heads_fused_ex\s*\(([^)]*)\)\s*;", header)
    assert m
    ctype_of = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}
    want = []
    for arg in m.group(1).split(","):
        words = arg.replace("*", " * ").split()
        if "*" in words:
            pointee = [w for w in words if w not in ("const", "*")][0]
            want.append({"xt_ppo_cfg": ctypes.POINTER(lib.PpoCfg)}.get(pointee, ctypes.c_void_p))
        else:
            want.append(ctype_of[[w for w in words if w != "const"][0]])
    res, args = lib.SIGNATURES["xt_ppo_gauss_heads_fused_ex"]
    assert res is ctypes.c_int32 and len(args) == len(want)
    for i, (a, w) in enumerate(zip(args, want)):
        assert a is w or (w is ctypes.c_void_p and a is ctypes.POINTER(ctypes.c_int32)), (i, a, w)
    # xt_tuning is untouched: the switch is per net
    assert [n for n, _ in lib.Tuning._fields_] == [
        "bf16x6", "dgrad_all_classes", "dgrad_tile64", "dgrad_halo", "bwd_own_instance", "bwd_fit_slots", "conv1_bf16x3",
        "conv1_flat", "conv1_waves", "fwd_two_groups", "direct", "direct_fwd", "direct_dgrad", "direct_all", "direct_waves",
        "direct_max_waves", "direct_tile64_tiles", "fwd_split_target", "wgrad_split_target", "reduce_z_lanes", "defer_splitk",
        "finalize_ticket", "fwd_tiled_valid", "wgrad_rows", "fwd_prefetch_all", "bwd_deep_prefetch", "fwd_four_groups",
        "reduce_deep_lanes", "fwd_xcd_chunk", "tail_overlap", "tail_fused", "dense_wgrad_x6", "fwd_fuse12", "bwd_fuse21"]


def test_gauss_head_entry_refuses_before_any_device_call():
    """(the checks run before the first device call, so they are tested where there is no GPU too)"""
    from xingtian_amd import lib
    h = lib.load()
    p = ctypes.c_void_p(4096)        # never dereferenced
    cfg = lib.PpoCfg()
    path = ctypes.c_int32(-1)

    def call(F, A, ks):
        part = p if ks else None
        return h.xt_ppo_gauss_heads_fused_ex(p, p, part, part, ks or 1, ks or 1, 8 * F, p, p, 1, 8, F, A, 0, p, p, p, p, p, None,
                                             p, p, p, p, p, ctypes.byref(cfg), 0.125, 1, p, p, p, p, p, (A + 3) // 4 * 4, p, p,
                                             p, p, p, None, None, ctypes.byref(path))

    for F, A, ks, msg in ((64, 9, 0, "A=9 F=64 ksplit=1/1"), (513, 4, 0, "A=4 F=513 ksplit=1/1"),
                          (64, 4, 17, "A=4 F=64 ksplit=17/17")):
        path.value = -1
        assert call(F, A, ks) != 0 and path.value == 0
        err = h.xt_last_error().decode()
        assert "xt_ppo_gauss_heads_fused_ex" in err and msg in err, err
    assert h.xt_net_set_gauss_fused(None, 1) != 0 and "xt_net_set_gauss_fused" in h.xt_last_error().decode()
