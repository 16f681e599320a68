"""CPU checks of the case tables of tests/test_gpu_optim_branch.py (the gradient-reduction launch, its four forms and the
optimisers of csrc/xt_optim.hip): the plans xt_grads_finish_plan_ex gives the tables cover every z-lane count, both sides of
every threshold the kernels branch on, every count % 4, every form with and without STATS and every optimiser; the entries
refuse bad arguments before any device call; and the comparison functions the GPU tests assert with reject a deliberately
wrong twin at every case it applies to.  A branch added without cases, or a comparison that stopped biting, fails here, on
any box."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def T():
    """the GPU module imported for its tables, twins and comparisons only (no test of it runs)"""
    spec = importlib.util.spec_from_file_location("_optim_cases", os.path.join(ROOT, "tests", "test_gpu_optim_branch.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def lib():
    from xingtian_amd import lib
    lib.load()
    return lib


def test_case_ids_are_unique(T):
    ids = [c.id for c in T.RED_CASES + T.FORM_CASES + T.OPT_CASES + T.KERAS_CASES]
    assert len(ids) == len(set(ids))
    assert {c.table for c in T.FORM_CASES} <= set(T.RED_BY_ID)


def test_plans_of_the_tables_cover_every_lane_count_threshold_and_tail(T, lib):
    defaults = lib.get_tuning()
    assert (defaults["reduce_z_lanes"], defaults["reduce_deep_lanes"]) == (8, 128)
    single, seen_zl = [], {}
    for c in T.RED_CASES:
        with T.Knobs(lib, c.knobs):
            arr, npart, grid = T.plan_of(lib, c)
        T.assert_plan(c, arr, npart)
        assert grid == c.grid and grid < 200, c.id
        for e in c.ents:
            seen_zl.setdefault(e.zl, set()).add(bool(c.knobs))
            assert e.nslab * (T.align4(e.count) + e.pad) <= 600000, c.id
        if len(c.ents) == 1:
            single.append(c.ents[0])
    assert lib.get_tuning() == defaults                                   # (every knob restored)
    assert {zl for zl, how in seen_zl.items() if False in how} == {1, 2, 4, 8, 32} and seen_zl[16] == {True}
    nslabs = {e.nslab for e in single}
    assert {1, 2, 5, 8, 9, 63, 64, 65, 127, 128, 250, 256, 257} <= nslabs
    assert any(e.inplace for e in single) and any(e.nslab == 1 and not e.inplace for e in single)
    assert {e.count for e in single if e.count < 8} >= {1, 2, 3, 4, 5, 7}
    every = [e for c in T.RED_CASES for e in c.ents]
    assert {e.count % 4 for e in every} == {0, 1, 2, 3}
    for zl in (1, 2, 4, 8, 16, 32):                                       # the block boundary of every lane count
        per = 4 * (256 // zl)
        assert any(e.zl == zl and e.count == per and e.nblk == 1 for e in every), zl
        assert any(e.zl == zl and e.count == per + 1 and e.nblk == 2 for e in every), zl
    assert any(2000 <= e.count <= 9000 for e in single) and any(e.pad > 0 for e in every) and any(e.pad == 0 for e in every)
    assert any(e.nslab == 8 * e.zl + 1 for e in every if e.zl in (8, 32))   # one slab into the second 8-deep round
    assert any(len(c.ents) == 12 for c in T.RED_CASES) and any(e.pre for e in every)
    assert any(c.early and len(c.ents) == 12 for c in T.RED_CASES)
    assert {1, 63, 64, 65} <= {c.grid for c in T.RED_CASES} and any(125 <= c.grid <= 135 for c in T.RED_CASES)


def test_form_and_optimiser_cases_cover_every_form_loss_block_and_size(T):
    F = T.FORM_CASES
    grids = {T.RED_BY_ID[c.table].grid for c in F}
    assert {1, 63, 64, 65} <= grids and any(g > 125 for g in grids)      # (+ 1 with the extra block: 64 | 65 | 66 as well)
    assert {c.n for c in F if c.loss == "ppo"} == {1, 255, 256, 257, 300}
    assert {(c.n, c.acc_set) for c in F if c.loss == "impala"} >= {(1, 1), (3, 0), (3, 1)}
    for loss in ("ppo", "impala"):                                        # every form runs for every case: form x STATS
        assert {c.stats for c in F if c.loss == loss} == {True, False}, loss
        assert {c.side for c in F if c.loss == loss and c.stats} == {"above", "below"} or loss == "impala"
    assert {c.side for c in F if c.stats} == {"above", "below"} and {c.lr_dev for c in F} == {True, False}
    assert any(any(e.pre for e in T.RED_BY_ID[c.table].ents) for c in F)
    assert any(any(e.zl == 32 for e in T.RED_BY_ID[c.table].ents) for c in F)
    O = T.OPT_CASES
    for kind in (T.OPT_ADAM, T.OPT_RMSPROP):
        mine = [c for c in O if c.opt == kind]
        assert {c.count for c in mine} == {1, 2, 3, 4, 5, 1003, T.BIG}, kind
        assert {c.side for c in mine} == {"below", "above", "zero"} and {c.stats for c in mine} == {True, False}
        assert {round(c.gs, 3) for c in mine} == {1.0, 0.5, 0.333}
    assert {c.npartial for c in O} == {1, 255, 256, 257, 2048, 2049, 2300}
    assert T.BIG > 512 * 256 * 4 and T.BIG > 2048 * 256 and T.BIG % 4 and T.BIG < 600000
    assert {c.lr_dev for c in O if c.opt == T.OPT_RMSPROP} == {True, False}
    assert (T.RMS_DECAY, T.RMS_EPS, T.OPT_STEPS) == (0.99, 0.1, 3) and 0.01 <= T.LR <= 0.1
    K = T.KERAS_CASES
    assert any(set(c.sizes) >= {1, 15, 16, 17, 4099} and max(c.sizes) > 512 * 256 for c in K)
    assert any(c.clipnorm == 0 for c in K) and any(len(c.sizes) == 32 for c in K)
    for c in K:
        d = T.keras_data(c)                                               # (asserts the side of every tensor, ratio 1.5)
        assert all(o % 4 for o, _ in d["segs"]) and (c.clipnorm == 0 or set(c.sides) == {0, 1}), c.id
    assert {n for n, _, _ in T.ADAM3_CASES} == {1, 2, 3, 4, 5, 1003, T.BIG}


def test_entries_refuse_before_any_device_call(T, lib):
    """(the checks run before the first device call, so they are tested where there is no GPU too)"""
    h = lib.load()
    err = lambda: h.xt_last_error().decode()
    npart, grid = ctypes.c_int32(-1), ctypes.c_int32(-1)

    def table(n=2, pre=0, src0=4096, stride=8):
        arr = (lib.GradEntry * n)()
        for i in range(n):
            arr[i].src, arr[i].dst, arr[i].count, arr[i].nslab, arr[i].stride = 4096 * (i + 1), 4096 * (i + 50), 5, 3, 8
        arr[0].src, arr[0].stride, arr[n - 1].pre = src0, stride, pre
        return arr

    def plan(arr, form=0, select=0, max_partials=64):
        return h.xt_grads_finish_plan_ex(arr, len(arr), select, 0, form, max_partials, ctypes.byref(npart), ctypes.byref(grid))

    assert plan(table()) == 0 and (npart.value, grid.value) == (2, 2)
    for kw, pkw, msg in ((dict(src0=4100), {}, "entry 0 not 16-byte aligned"), (dict(stride=6), {}, "entry 0 not 16-byte aligned"),
                         ({}, dict(form=1, select=1), "last-block finalize form needs the whole table"),
                         (dict(pre=2), dict(form=1), "last-block finalize form needs the whole table"),
                         ({}, dict(form=3, select=2), "fused tail takes the whole table"),
                         ({}, dict(max_partials=1), "2 partial blocks > scratch 1"), ({}, dict(form=4), "form 4 outside")):
        assert plan(table(**kw), **pkw) != 0 and (npart.value, grid.value) == (0, 0), msg
        assert msg in err(), err()
    # the launch entry: the same refusals, and the fused tail without its barrier scratch
    p = 8192
    form_out = ctypes.c_int32(7)

    def launch(arr, select=0, **kw):
        a = lib.FinishArgs()
        a.partial, a.max_partials, a.state, a.clip_norm, a.grad_scale = p, 64, p, 1.0, 1.0
        a.params = a.m = a.v = a.grads_base = 4096
        for k, v in kw.items():
            setattr(a, k, v)
        return h.xt_grads_finish_ex(arr, len(arr), select, 0, ctypes.byref(a), None, ctypes.byref(form_out), None)

    for kw, skw, msg in ((dict(src0=4100), dict(form=0), "not 16-byte aligned"), ({}, dict(form=1, counter=p, select=1), "whole table"),
                         ({}, dict(form=1), "needs the ticket counter"), ({}, dict(form=3), "fused tail takes the whole table and a barrier"),
                         ({}, dict(form=3, counter=p, select=1), "fused tail takes the whole table"),
                         ({}, dict(form=2, max_partials=1), "partial blocks > scratch"),
                         ({}, dict(form=2, terms=p, B=0), "B=0")):
        select = skw.pop("select", 0)
        assert launch(table(**kw), select, **skw) != 0 and form_out.value == -1, msg
        assert "grads_finish" in err() and msg in err(), err()
    # optimisers
    n = 33
    off, size = (ctypes.c_int64 * n)(*range(n)), (ctypes.c_int64 * n)(*([1] * n))
    assert h.xt_adam_keras(p, p, p, p, n, off, size, 1.0, 0.01, 0.9, 0.999, 1e-7, p, None) != 0 and "n_seg 33" in err()
    assert h.xt_optim_clip_ex(T.OPT_ADAM, p + 4, p, p, p, 8, 0.1, None, 0.9, 0.999, 1e-7, p, p, 1, 1.0, 1.0, None, None) != 0
    assert "16-byte aligned" in err()
    assert h.xt_optim_clip_ex(2, p, p, p, p, 8, 0.1, None, 0.9, 0.999, 1e-7, p, p, 1, 1.0, 1.0, None, None) != 0
    assert "unknown opt_type" in err()
    assert h.xt_norm_finalize_ex(p, 0, ctypes.byref(lib.FinishArgs()), None) != 0 and "xt_norm_finalize_ex" in err()


CTYPE_OF = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32, "float": ctypes.c_float}


def test_entries_and_structs_are_bound_with_the_headers_declarations(lib):
    header = open(os.path.join(ROOT, "include", "xt_mi355x.h")).read()
    assert re.search(r"#define XT_ABI_VERSION 12\b", header) and lib.ABI_VERSION == 12
    structs = {"xt_grad_entry": lib.GradEntry, "xt_finish_args": lib.FinishArgs}
    for name, cls in structs.items():
        body = re.search(r"typedef struct {0} \{{(.*?)\}} {0};".format(name), header, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        want = []
        for decl in body.split(";"):
            words = decl.replace("*", " * ").replace(",", " , ").split()
            if not words:
                continue
            base = [w for w in words if w != "const"][0]
            names, star = [], False
            for w in words[words.index(base) + 1:]:
                if w == "*":
                    star = True
                elif w != ",":
                    names.append((w, ctypes.c_void_p if star else CTYPE_OF[base]))
                    star = False
            want += names
        assert [(n, t) for n, t in cls._fields_] == want, name
    for name in ("xt_grads_finish_plan_ex", "xt_grads_finish_ex", "xt_optim_clip_ex", "xt_norm_finalize_ex"):
        m = re.search(r"\bint\s+{}\s*\(([^)]*)\)\s*;".format(name), header)
        assert m, name
        want = []
        for arg in m.group(1).split(","):
            words = arg.replace("*", " * ").split()
            if "*" in words:
                pointee = [w for w in words if w not in ("const", "*")][0]
                want.append(ctypes.POINTER(structs[pointee]) if pointee in structs else ctypes.c_void_p)
            else:
                want.append(CTYPE_OF[[w for w in words if w != "const"][0]])
        res, args = lib.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(args) == len(want), name
        for i, (a, w) in enumerate(zip(args, want)):
            assert a is w or (w is ctypes.c_void_p and a is ctypes.POINTER(ctypes.c_int32)), (name, i, a, w)
        assert hasattr(lib.load(), name)
    assert "xt_grads_finish_plan_ex" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


# ---------------------------------------------------------------- the comparisons bite
def test_reduction_comparisons_reject_a_dropped_slab_lane_or_tail(T):
    applied = {"last_slab": 0, "float4_lane": 0, "tail": 0}
    for c in T.RED_CASES:
        d = T.red_data(c)
        ref = T.red_reference(c, d)
        for bug in applied:
            wrong = T.red_reference(c, d, bug)
            for i, e in enumerate(c.ents):
                if e.inplace or (bug == "tail" and e.count % 4 == 0):
                    continue
                applied[bug] += 1
                assert T.bits_differ(wrong["twin"][i], ref["twin"][i]) > 0, (c.id, i, bug)
                assert not T.within(T.rel2(wrong["twin"][i], ref["ref64"][i]), T.BAR_ELEM), (c.id, i, bug)
                if not e.pre:
                    sl = slice(c.pblk0[i], c.pblk0[i] + e.nblk)
                    assert not T.within(T.slots_err(wrong["partial"][sl], ref["partial"][sl]), T.BAR_ELEM), (c.id, i, bug)
        # ... and the float32 twin itself lies well inside the bar (the ordered sum against float64)
        for t, r in zip(ref["twin"], ref["ref64"]):
            assert T.rel2(t, r) < 0.25 * T.BAR_ELEM, c.id
    assert min(applied.values()) >= 20, applied


def test_norm_and_update_comparisons_reject_a_dropped_partial_a_missing_grad_scale_and_a_stale_beta_power(T):
    n_partial = n_gs = n_beta = 0
    for c in T.OPT_CASES:
        d = T.opt_data(c)
        state = np.array([1, 1, 0, 0, 0, 0, 0, 0], np.float32)
        p, m, v = d["p"], d["m"], d["v"]             # (carried from step to step by the float32 oracle, as a device would)
        for k in range(T.OPT_STEPS):
            gn, sc = T.clip_ref(d["partial"][k], T.OPT_CLIP, c.gs)
            b1p, b2p, alpha, cnt = T.advance_ref(state, T.LR)
            step = (lambda s, a: T.adam_ref(p, d["g"][k], m, v, s, a)) if c.opt == T.OPT_ADAM else \
                (lambda s, a: T.rmsprop_ref(p, d["g"][k], m, v, s, T.LR))
            good = step(sc, alpha)
            # the float32 build of the oracle stays an order of magnitude inside the bars
            gn32, sc32 = T.clip_ref(d["partial"][k], T.OPT_CLIP, c.gs, np.float32)
            _, _, a32, _ = T.advance_ref(state, T.LR, np.float32)
            o32 = T.adam_ref(p, d["g"][k], m, v, sc32, a32, np.float32) if c.opt == T.OPT_ADAM else \
                T.rmsprop_ref(p, d["g"][k], m, v, sc32, T.LR, np.float32)
            assert max(T.rel2(x, y) for x, y in zip(o32, good)) < 0.25 * T.BAR_ELEM, (c.id, k)
            assert max(T.rel1(gn32, gn), T.rel1(sc32, sc), T.rel1(a32, alpha)) < 0.1 * T.BAR_NORM, (c.id, k)
            if c.npartial > 1 and c.side != "zero":
                n_partial += 1
                gw, sw = T.clip_ref(d["partial"][k], T.OPT_CLIP, c.gs, bug="last_partial")
                assert not T.within(T.rel1(gw, gn), T.BAR_NORM), (c.id, k)
                if c.side == "above":      # (below the clip norm the factor does not depend on the norm)
                    assert not T.within(T.rel1(sw, sc), T.BAR_NORM), (c.id, k)
                    # (Adam's step is nearly invariant to the gradient's scale: a wrong factor shows in m and v)
                    wrong = step(sw, alpha)
                    assert not T.within(T.rel2(wrong[0], good[0]), T.BAR_ELEM) and not T.within(T.rel2(wrong[1], good[1]), T.BAR_ELEM), c.id
            if abs(c.gs - 1.0) > 0.1 and c.side != "zero":
                n_gs += 1
                _, sw = T.clip_ref(d["partial"][k], T.OPT_CLIP, c.gs, bug="grad_scale")
                assert not T.within(T.rel1(sw, sc), T.BAR_NORM), (c.id, k)
                wrong = step(sw, alpha)
                assert not T.within(T.rel2(wrong[0], good[0]), T.BAR_ELEM) and not T.within(T.rel2(wrong[1], good[1]), T.BAR_ELEM), c.id
                if c.opt == T.OPT_RMSPROP:
                    assert not T.within(T.rel2(wrong[2], good[2]), T.BAR_ELEM), c.id
            if c.opt == T.OPT_ADAM:
                n_beta += 1
                w1, w2, aw, _ = T.advance_ref(state, T.LR, bug="beta_power")
                assert T.bits_differ(np.array([w1, w2]), np.array([b1p, b2p])) == 2, (c.id, k)
                assert not T.within(T.rel1(aw, alpha), T.BAR_NORM), (c.id, k)
                if c.side != "zero":
                    assert not T.within(T.rel2(step(sc, aw)[2], good[2]), T.BAR_ELEM), (c.id, k)
            state = np.array([b1p, b2p, sc, alpha, gn, cnt, 0, 0], np.float32)
            p, m, v = p + o32[2], o32[0], o32[1]
    assert n_partial >= 20 and n_gs >= 20 and n_beta >= 20, (n_partial, n_gs, n_beta)


def test_keras_comparison_rejects_a_tensor_clipped_with_its_neighbours_norm(T):
    applied = 0
    for c in T.KERAS_CASES:
        d = T.keras_data(c)
        ins = d["inside"]
        p, m, v = d["p"], d["m"], d["v"]
        for k in range(T.OPT_STEPS):
            lr_t = T.keras_lr_t(k + 1)
            good = T.keras_ref(p, d["g"][k], m, v, d["segs"], c.clipnorm, lr_t)
            o32 = T.keras_ref(p, d["g"][k], m, v, d["segs"], c.clipnorm, lr_t, np.float32)
            assert max(T.rel2(x[ins], y[ins]) for x, y in zip(o32, good)) < 0.25 * T.BAR_ELEM, (c.id, k)
            if c.clipnorm > 0:
                applied += 1
                wrong = T.keras_ref(p, d["g"][k], m, v, d["segs"], c.clipnorm, lr_t, bug="neighbour_norm")
                for x, y in list(zip(wrong, good))[:2]:      # (m and v: Adam's step is nearly invariant to the gradient's scale)
                    assert not T.within(T.rel2(x[ins], y[ins]), T.BAR_ELEM), (c.id, k)
            p, m, v = np.where(ins, p + o32[2], p).astype(np.float32), o32[0], o32[1]
    assert applied >= 6


def test_loss_references_in_float32_stay_inside_the_loss_bar(T):
    for c in T.FORM_CASES:
        fd = T.form_data(c)
        if c.loss == "ppo":
            l64, _ = T.ppo_loss_ref(fd["terms"], T.PPO_ENT, T.PPO_CRITIC, fd["inv_b"])
            l32, _ = T.ppo_loss_ref(fd["terms"], T.PPO_ENT, T.PPO_CRITIC, fd["inv_b"], np.float32)
            assert max(T.rel1(a, b) for a, b in zip(l32, l64)) < 0.1 * T.BAR_LOSS, c.id
            assert min(abs(l64)) > 0.1, c.id                              # (no cancellation: a relative bar is meaningful)
