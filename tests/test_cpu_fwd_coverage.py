"""CPU checks that the case tables of tests/test_gpu_fwd_layer.py cover the forward dispatcher and the first layer's
weight-gradient dispatcher: every XT_FWD_PATH_* / XT_WG1_PATH_* branch include/xt_mi355x.h declares has cases at two
geometries or more, a one-entry probe and a random-data case; every first-layer branch is run gathered and at one sample;
every non-default value of the knobs the dispatchers read is run once; both sides of the batch thresholds are there.  A
branch added to the header without cases fails here, on any box."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    """the GPU module imported for its tables only (nothing of it runs)"""
    spec = importlib.util.spec_from_file_location("_fwd_cases", os.path.join(ROOT, "tests", "test_gpu_fwd_layer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def geometry(c):
    return (c.kind, c.hw, c.cin, c.cout, c.k, getattr(c, "kh", None), c.s, c.padding)


def check_paths(paths, cases, what):
    assert len(set(paths.values())) == len(paths) and 0 not in paths.values()      # (0 = "no launch recorded")
    for c in cases:
        assert c.path in paths, (c.id, c.path)
    for name in paths:
        mine = [c for c in cases if c.path == name]
        assert len(mine) >= 2, "{}{}: fewer than two cases".format(what, name)
        assert len({geometry(c) for c in mine}) >= 2, "{}{}: a single geometry".format(what, name)
        assert any(c.probe for c in mine), "{}{}: no probe case".format(what, name)
        assert any(not c.probe for c in mine), "{}{}: no random-data case".format(what, name)


def test_every_fwd_and_wg1_branch_has_cases_at_two_geometries_and_a_probe(T):
    assert len(T.fwd_paths()) >= 7 and len(T.wg1_paths()) >= 4
    check_paths(T.fwd_paths(), T.FWD_CASES, "XT_FWD_PATH_")
    check_paths(T.wg1_paths(), T.WG1_CASES, "XT_WG1_PATH_")
    ids = [c.id for c in T.FWD_CASES + T.WG1_CASES]
    assert len(ids) == len(set(ids))
    tiles = T.header_defines("XT_FWD_TILE_")
    for c in T.FWD_CASES:
        assert c.tile == 0 or c.tile in tiles, c.id
        assert c.path in T.ARITH_OF and c.act in ("relu", "none", "elu", "tanh"), c.id
        assert (c.tile == 0) == c.path.startswith("C1_"), c.id
        assert c.probe is False or (c.act == "none" and not c.gather), c.id
        assert c.gather is False or c.xform[0] == 1, c.id            # (the row gather reads a uint8 pool)
    assert {"relu", "none", "elu"} <= {c.act for c in T.FWD_CASES if c.path in ("C1_FLAT", "C1_STACK")}
    for c in T.WG1_CASES:
        assert c.msplit <= c.slab_cap and c.xform[0] == 1, c.id
    # every tile shape and unit count the header documents is expected by some row
    assert {c.tile for c in T.FWD_CASES if c.tile} == set(n for n in tiles if n != "SHIFT")
    assert {1, 2, 4} <= {c.units for c in T.FWD_CASES if c.path == "TILED_X6"}
    assert {1, 2} <= {c.units for c in T.FWD_CASES if c.path == "TILED_FP32"}
    for cases in (T.FWD_CASES, T.WG1_CASES):
        assert {4, 8} <= {c.units for c in cases if c.path == "C1_STACK"}
        assert {256, 512} <= {c.units for c in cases if c.path == "C1_SAME"}
    assert {256, 512} <= {c.units for c in T.FWD_CASES if c.path == "C1_FLAT"}


def test_first_layer_branches_run_gathered_and_at_one_sample(T):
    for name in ("C1_FLAT", "C1_STACK", "C1_SAME"):
        for cases, what in ((T.FWD_CASES, "forward"), (T.WG1_CASES, "weight gradient")):
            mine = [c for c in cases if c.path == name]
            assert any(c.gather for c in mine), (what, name, "no gathered case")
            if (what, name) != ("weight gradient", "C1_FLAT"):      # (that form needs 200 blocks of 512 positions)
                assert any(c.B == 1 for c in mine), (what, name, "no B = 1 case")
    # the SAME form with an integer mean, gathered and not; the relu sign mask on both slot counts of the flattened form
    for cases in (T.FWD_CASES, T.WG1_CASES):
        m128 = [c for c in cases if c.path == "C1_SAME" and c.xform[1] == 128.0]
        assert any(c.gather for c in m128) and any(not c.gather for c in m128)
    assert {256, 512} <= {c.units for c in T.FWD_CASES if c.path == "C1_FLAT" and c.act == "relu"}
    # one block writes dwb directly; one frame stack does too
    assert any(c.path == "C1_SAME" and c.slabs == 1 for c in T.WG1_CASES)
    assert any(c.path == "C1_STACK" and c.slabs == 1 for c in T.WG1_CASES)
    # the slab capacity: exactly enough, one short (generic), and fewer than the SAME form's blocks (generic)
    assert any(c.path == "C1_STACK" and c.B == c.slab_cap > 1 for c in T.WG1_CASES)
    assert any(c.path == "GENERIC" and c.padding == "valid" and c.B == c.slab_cap + 1 and not c.knobs for c in T.WG1_CASES)
    assert any(c.path == "GENERIC" and c.padding == "same" and not c.knobs for c in T.WG1_CASES)
    assert {1, 5} <= {c.msplit for c in T.WG1_CASES if c.path == "GENERIC" and c.knobs.get("conv1_bf16x3") == 0}


def test_fwd_cases_cover_knobs_prefetch_instances_and_thresholds(T):
    from xingtian_amd import lib
    fields = {n for n, _ in lib.Tuning._fields_}
    seen = {}
    for c in T.FWD_CASES + T.WG1_CASES:
        for k, v in c.knobs.items():
            assert k in fields, (c.id, k)
            seen.setdefault(k, set()).add(v)
    want = {"conv1_bf16x3": [0], "conv1_flat": [0], "conv1_waves": [4], "fwd_two_groups": [0], "fwd_four_groups": [0],
            "fwd_prefetch_all": [1], "fwd_xcd_chunk": [0], "fwd_tiled_valid": [0], "direct": [0], "direct_fwd": [0],
            "direct_all": [1], "bf16x6": [0]}
    assert T.KNOBS == want
    defaults = lib.get_tuning()
    for k, values in T.KNOBS.items():
        assert k in fields, k
        for v in values:
            assert v in seen.get(k, ()), "tuning {} = {} has no case".format(k, v)
            assert defaults[k] != v, "tuning {} = {} is the default".format(k, v)
    # the first-layer knobs are run by both tables
    for k in ("conv1_bf16x3", "conv1_flat", "conv1_waves"):
        for cases in (T.FWD_CASES, T.WG1_CASES):
            assert any(k in c.knobs for c in cases), k
    # all five all-loads-up-front instances, and a launch that falls through to the grouped form
    inst = {(c.nst, c.tile) for c in T.FWD_CASES if c.path == "TILED_X6_ALL"}
    assert inst == {(4, "128X32"), (4, "64X64"), (5, "64X64"), (8, "128X32"), (8, "64X64")}
    assert any(c.path == "TILED_X6" and c.knobs.get("fwd_prefetch_all") == 1 for c in T.FWD_CASES)
    # thresholds, both sides: 200 blocks of 512 positions (first layer), 256 / 320 blocks (wave groups)
    by = lambda cases, name, hw: {c.B: c.units for c in cases if c.path == name and c.hw == hw and not c.knobs}
    f = by(T.FWD_CASES, "C1_FLAT", (84, 84))
    assert (f.get(254), f.get(255)) == (256, 512)
    s = by(T.FWD_CASES, "C1_SAME", (84, 84))
    assert (s.get(231), s.get(232)) == (256, 512)
    assert by(T.WG1_CASES, "C1_STACK", (84, 84)).get(254) == 8 and by(T.WG1_CASES, "C1_FLAT", (84, 84)).get(255) == 512
    s = by(T.WG1_CASES, "C1_SAME", (84, 84))
    assert (s.get(231), s.get(232)) == (256, 512)

    def blocks(c):
        lay = T.layer_of(c)
        m = c.B * lay.out_h * lay.out_w
        return (-(-m // 128) if c.cout <= 32 else -(-m // 64) * -(-c.cout // 64)) * c.ks
    groups = {(c.tile, blocks(c)): c.units for c in T.FWD_CASES if c.path == "TILED_X6" and not c.knobs}
    assert (groups.get(("128X32", 256)), groups.get(("128X32", 257))) == (4, 2)
    assert (groups.get(("128X32", 320)), groups.get(("128X32", 321))) == (2, 1)
    assert (groups.get(("64X64", 320)), groups.get(("64X64", 321))) == (2, 1)
    # split-K: a request the dispatcher lowers, and the register-direct kernel's own split
    assert any(c.path == "TILED_X6" and 1 < c.ks < c.ksplit for c in T.FWD_CASES)
    assert any(c.path == "DIRECT" and c.ks > 1 for c in T.FWD_CASES)
    assert any(c.kind == "dense" and c.B == 1 for c in T.FWD_CASES)
    assert sum(c.B >= 254 for c in T.FWD_CASES + T.WG1_CASES) <= 8


def test_wgrad_slabs_refuses_a_split_beyond_the_slab_capacity():
    """(the check runs before any device call, so it is tested where there is no GPU too)"""
    import ctypes
    from xingtian_amd import lib
    g = lib.ConvGeom(84, 84, 4, 8, 8, 4, 0, 0, 20, 20, 32, 1)
    xf = lib.InputXform(1, 0.0, 255.0)
    path = ctypes.c_int32(-1)
    for slabs, cap, msplit in ((None, 8, 2), (ctypes.c_void_p(4096), 4, 5)):
        rc = lib.load().xt_layer_wgrad_slabs(ctypes.byref(g), ctypes.byref(xf), 5, None, None, None, None, slabs, cap, msplit,
                                             None, ctypes.byref(path))
        assert rc != 0 and path.value == 0
        assert "xt_layer_wgrad_slabs: msplit {}".format(msplit) in lib.load().xt_last_error().decode()
