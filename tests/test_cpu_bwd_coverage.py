"""CPU checks that the case table of tests/test_gpu_bwd_layer.py covers the fused backward launch's dispatch: every
XT_BWD_PATH_* branch include/xt_mi355x.h declares has cases at two geometries or more and a one-entry probe, and every
documented non-default tuning value is run once.  A branch added to the header without cases fails here, on any box."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    """the GPU module imported for its table only (nothing of it runs)"""
    spec = importlib.util.spec_from_file_location("_bwd_cases", os.path.join(ROOT, "tests", "test_gpu_bwd_layer.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def geometry(c):
    return (c.kind, c.hw, c.cin, c.cout, c.k, c.s, c.padding)


def test_every_bwd_branch_has_cases_at_two_geometries_and_a_probe(T):
    paths = T.header_paths()
    assert len(paths) >= 12 and len(set(paths.values())) == len(paths)
    assert 0 not in paths.values()          # (0 = "no launch recorded")
    ids = [c.id for c in T.BWD_CASES]
    assert len(ids) == len(set(ids))
    for c in T.BWD_CASES:
        assert c.path in paths, (c.id, c.path)
        assert c.dg in range(6), c.id
        assert c.act in ("relu", "relu_mask", "tanh", "swish", "gelu", "none"), c.id
    for name in paths:
        mine = [c for c in T.BWD_CASES if c.path == name]
        assert len(mine) >= 2, "XT_BWD_PATH_{}: fewer than two cases".format(name)
        assert len({geometry(c) for c in mine}) >= 2, "XT_BWD_PATH_{}: a single geometry".format(name)
        assert any(c.probe for c in mine), "XT_BWD_PATH_{}: no probe case".format(name)
        assert any(not c.probe for c in mine), "XT_BWD_PATH_{}: no random-data case".format(name)


def test_bwd_cases_cover_knobs_activations_and_batch_edges(T):
    from xingtian_amd import lib
    fields = {n for n, _ in lib.Tuning._fields_}
    seen = {}
    for c in T.BWD_CASES:
        for k, v in c.knobs.items():
            assert k in fields, (c.id, k)
            seen.setdefault(k, set()).add(v)
    for k, values in T.KNOBS.items():
        assert k in fields, k
        for v in values:
            assert v in seen.get(k, ()), "tuning {} = {} has no case".format(k, v)
    acts = {c.act for c in T.BWD_CASES}
    assert {"relu", "relu_mask", "tanh", "none"} <= acts and acts & {"swish", "gelu"}
    # the relu mask is read by the all-classes input gradients only: every one of those branches runs with it
    for name in ("CLASSES_PF4", "CLASSES_WROWS", "CLASSES"):
        assert any(c.path == name and c.act == "relu_mask" for c in T.BWD_CASES), name
    by = lambda name: {c.B for c in T.BWD_CASES if c.path == name}
    assert {511} <= by("S2C16") and {512} <= by("S2FUSED")
    assert any(c.path == "S2C16" and c.B >= 512 and c.slab_cap is not None and c.slab_cap < 512 for c in T.BWD_CASES)
    assert {614} <= by("CLASSES_PF4") and {615} <= by("CLASSES") and {384} <= by("PF_GENERIC") and \
        {385} <= by("PAIR_LL_WX6")
    for name in T.header_paths():
        if name not in ("HALO", "S2FUSED"):        # (both need hundreds of samples to be selected at all)
            assert 1 in by(name), "XT_BWD_PATH_{}: no B = 1 case".format(name)
