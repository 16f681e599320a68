"""CPU checks that the case tables of tests/test_gpu_heads_branch.py cover the fused head kernels: every XT_HEAD_PATH_*
family include/xt_mi355x.h declares and every NQ x PART x SHARED (PPO), NQ x PART and AM (IMPALA) instance has cases at
two geometries or more, a probe and a random-data case; both sides of every threshold are there; the float64 reference
of every PPO case, re-run here, populates all four gradient outcomes and leaves out at most 2 % of the rows; the
geometries the kernels refuse are refused before any device call.  An instance added without cases fails here, on any
box."""
import ctypes
import importlib.util
import itertools
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    """the GPU module imported for its tables and its numpy references only (no test of it runs)"""
    spec = importlib.util.spec_from_file_location("_heads_cases", os.path.join(ROOT, "tests", "test_gpu_heads_branch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def covered(rows, what):
    assert len(rows) >= 2, what + ": fewer than two cases"
    assert len({(c.F, c.A, getattr(c, "B", None), getattr(c, "T", None), getattr(c, "n_traj", None)) for c in rows}) >= 2, \
        what + ": a single geometry"
    assert any(c.probe for c in rows), what + ": no probe case"
    assert any(not c.probe for c in rows), what + ": no random-data case"


def test_every_head_instance_has_cases_at_two_geometries_and_a_probe(cases):
    paths = cases.head_paths()
    assert set(paths) == {"PPO_FUSED", "IMPALA"} and sorted(paths.values()) == [1, 2]      # (0 = "nothing launched")
    ids = [c.id for c in cases.PPO_CASES + cases.IMPALA_CASES + cases.WG_CASES]
    assert len(ids) == len(set(ids))
    # The instance lists below (NQ 1 / 2 / 4 / 8, PART, SHARED, AM 8 / 32) and nq_of restate the dispatch of
    # launch_ppo_heads_fused, launch_impala_heads_fwd and launch_impala_vtrace_bwd (csrc/xt_heads.hip): an instance
    # added there needs its row here and its cases in the tables.
    nq_of = lambda f: 1 if f <= 64 else 2 if f <= 128 else 4 if f <= 256 else 8
    for c in cases.PPO_CASES:
        assert c.nq == nq_of(c.F) and c.B <= 40 and c.A <= 8 and c.F <= 512, c.id
    for c in cases.IMPALA_CASES:
        assert c.nq == (nq_of(c.F) if c.fwd else 0) and c.am == (8 if c.A <= 8 else 32) and c.n_traj <= 3, c.id
        assert c.fwd or not c.ks, c.id
    covered(cases.PPO_CASES, "XT_HEAD_PATH_PPO_FUSED")
    covered(cases.IMPALA_CASES, "XT_HEAD_PATH_IMPALA")
    for nq, part, shared in itertools.product((1, 2, 4, 8), (False, True), (False, True)):
        covered([c for c in cases.PPO_CASES if (c.nq, bool(c.ks), c.shared) == (nq, part, shared)],
                "ppo_heads_fused_kernel<{}, {}, {}>".format(nq, part, shared))
    for nq, part in itertools.product((1, 2, 4, 8), (False, True)):
        mine = [c for c in cases.IMPALA_CASES if (c.nq, bool(c.ks)) == (nq, part)]
        covered(mine, "impala_heads_fwd_kernel<{}, {}>".format(nq, part))
        assert any(c.probe == "fwd" for c in mine), (nq, part)
    for am in (8, 32):
        mine = [c for c in cases.IMPALA_CASES if c.am == am]
        covered(mine, "impala_vtrace_bwd_kernel<{}>".format(am))
        assert any(c.probe == "vtrace" for c in mine), am


def test_head_cases_hold_the_parameter_values_and_both_sides_of_every_threshold(cases):
    P, I, W = cases.PPO_CASES, cases.IMPALA_CASES, cases.WG_CASES
    # ---- PPO
    assert {c.F for c in P} == {1, 37, 64, 65, 100, 128, 200, 256, 300, 512}        # 64|65, 128|200, 256|300 by NQ
    assert {c.A for c in P} == {1, 2, 5, 8} and {c.B for c in P} == {1, 3, 40}
    assert {k for c in P if c.ks for k in c.ks} == {1, 2, 3, 5, 16}
    assert any(c.ks and not c.shared and c.ks[0] != c.ks[1] and not c.probe for c in P)
    for sel in (lambda c: not c.ks, lambda c: bool(c.ks)):
        assert {"relu", "tanh"} <= {c.act for c in P if sel(c) and not c.probe}
    assert any(c.idx for c in P) and any(not c.idx for c in P) and cases.POOL_EXTRA > 0
    assert sum(c.inv_b_mul == 0.5 for c in P) == 1 and all(c.inv_b_mul in (0.5, 1.0) for c in P)
    for c in P:
        assert not c.probe or (c.act == "relu" and c.A <= 2 and (c.shared or c.A == 2)), c.id
    # ---- IMPALA
    assert {c.T for c in I} == {2, 8, 9, 63, 64, 65, 128, 129, 193, 256}              # 64|65, 128|129, 192|193, 256
    assert {c.n_traj for c in I} == {1, 3} and {c.F for c in I} == {5, 64, 100, 256, 300, 512, 128, 200}
    assert {c.A for c in I if c.am == 8} == {1, 3, 8} and {c.A for c in I if c.am == 32} == {9, 18, 32}     # 8|9
    assert {c.ks for c in I if c.ks} == {2, 16}
    assert {c.done for c in I if not c.probe} == {"none", "all", "last", "random"}
    assert any(c.T % 8 for c in I) and any(c.F >= 256 and c.T > 8 for c in I) and any(c.F < 64 for c in I)
    for am in (8, 32):
        assert any(c.T == 256 for c in I if c.am == am) and any(c.T > 64 and c.T % 64 for c in I if c.am == am)
    # ---- head weight-gradient slabs
    assert {c.B for c in W} == {1, 7, 8, 9, 40} and {c.F for c in W} == {1, 63, 64, 65, 200}
    assert {c.A for c in W} == {1, 7, 8, 9, 18} and {c.shared for c in W} == {True, False}
    assert any(c.probe for c in W)


def test_ppo_references_populate_every_gradient_branch_and_exclude_few_rows(cases):
    for c in cases.PPO_CASES:
        d = cases.ppo_data(c)
        ref = cases.ppo_reference(c, d)
        keep = ref["keep"]
        assert keep.any() and (~keep).sum() <= 0.02 * c.B, (c.id, int((~keep).sum()))
        for k in ("logits", "value", "dlogits", "dvalue", "terms"):
            assert np.isfinite(ref[k]).all(), (c.id, k)
        if c.idx:
            assert len(set(d["idx"].tolist())) == c.B and d["idx"].max() >= c.B and len(d["action"]) > c.B, c.id
        if c.B >= 30 and not c.probe:
            for k, v in ref["pops"].items():
                assert v >= 0.10, (c.id, k, v)
        if c.probe:          # the sign pattern the 2-ulp bound of the probed d(features) entries rests on
            col = (7 * np.arange(c.B) + 3) % c.F
            dl = ref["dlogits"]
            act = d["action"][d["rows"]]
            for b in range(c.B):
                terms = dl[b] * d["wpi"][col[b]]
                assert (terms <= 0).all() and ref["dvalue"][b] * d["wv"][col[b]] < 0, (c.id, b)
                assert c.A == 1 or dl[b, act[b]] < 0, (c.id, b)
            assert ref["pops"]["dsurr_adv"] == 1.0 and ref["pops"]["dv_live"] == 1.0, c.id


def test_head_entries_refuse_before_any_device_call():
    """(the checks run before the first device call, so they are tested where there is no GPU too)"""
    from xingtian_amd import lib
    h = lib.load()
    p = ctypes.c_void_p(4096)        # never dereferenced
    cfg = lib.PpoCfg()
    path = ctypes.c_int32(-1)

    def ppo(F, A, ks):
        part = p if ks else None
        return h.xt_ppo_heads_fused_ex(p, p, part, part, ks or 1, ks or 1, 8 * F, p, p, 1, 8, F, A, 0, p, p, p, p, None, p, p,
                                       p, p, p, ctypes.byref(cfg), 0.125, 1, p, p, p, p, p, p, p, p, p, None,
                                       ctypes.byref(path))

    for F, A, ks, msg in ((64, 9, 0, "A=9 F=64 ksplit=1/1"), (513, 4, 0, "A=4 F=513 ksplit=1/1"),
                          (64, 4, 17, "A=4 F=64 ksplit=17/17")):
        path.value = -1
        assert ppo(F, A, ks) != 0 and path.value == 0
        err = h.xt_last_error().decode()
        assert "xt_ppo_heads_fused_ex" in err and msg in err, err

    def impala(tlen, A, run_fwd):
        return h.xt_impala_heads_ex(p, None, 1, 0, None, 1, run_fwd, 1, tlen, 64, A, p, p, p, p, p, p, p, p, 0.99, 1, None, p, p,
                                    p, p, p, p, p, p, p, None, ctypes.byref(path))

    for tlen, A, run_fwd, msg in ((257, 4, 1, "T=257 A=4"), (9, 33, 0, "T=9 A=33"), (9, 9, 1, "A=9 F=64 ksplit=1")):
        path.value = -1
        assert impala(tlen, A, run_fwd) != 0 and path.value == 0
        err = h.xt_last_error().decode()
        assert "xt_impala_heads_ex" in err and msg in err, err
    n = ctypes.c_int32(-1)
    assert h.xt_heads_wgrad_partial_ex(p, p, 9, 64, 4, p, p, p, 64 * 4 + 3, p, 65, ctypes.byref(n), None) != 0 and n.value == 0
    assert "slab strides" in h.xt_last_error().decode()


CTYPE_OF = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "float": ctypes.c_float}


def test_head_entries_are_bound_with_the_headers_signatures():
    """the prototypes of xingtian_amd.lib against the declarations of include/xt_mi355x.h, argument by argument"""
    from xingtian_amd import lib
    header = open(os.path.join(ROOT, "include", "xt_mi355x.h")).read()
    for name in ("xt_ppo_heads_fused_ex", "xt_impala_heads_ex", "xt_heads_wgrad_partial_ex"):
        m = re.search(r"\bint\s+{}\s*\(([^)]*)\)\s*;".format(name), header)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            words = arg.replace("*", " * ").split()
            if "*" in words:
                pointee = [w for w in words if w not in ("const", "*")][0]
                want.append({"xt_ppo_cfg": ctypes.POINTER(lib.PpoCfg)}.get(pointee, ctypes.c_void_p))
            else:
                want.append(CTYPE_OF[[w for w in words if w != "const"][0]])
        res, args = lib.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(args) == len(want), name
        for i, (a, w) in enumerate(zip(args, want)):
            # (an int32 out-parameter is bound as POINTER(c_int32), every other pointer as void*)
            ok = a is w or (w is ctypes.c_void_p and a is ctypes.POINTER(ctypes.c_int32))
            assert ok, (name, i, a, w)
        assert hasattr(lib.load(), name)
