"""CPU side of the train-entry tables (tests/train_entry_helpers.py): every scalar field of the two cfg structs and every
data pointer of the two train prototypes, parsed out of include/xt_mi355x.h, has a key-mutation row (or is one of the two
named exemptions); the loop tables hold both sides of every condition of the two loops and their literal step counts
agree with the loop arithmetic restated in Python; every near-collision row really collides under ``"%g"`` and really
differs as float32; the cache report is bound with the header's signature."""
import ctypes
import os
import re

import numpy as np
import pytest

import train_entry_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "include", "xt_mi355x.h")) as _f:
    HEADER = re.sub(r"/\*.*?\*/", " ", _f.read(), flags=re.S)


def struct_fields(name):
    """scalar field names of ``typedef struct name { ... } name;`` in declaration order"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            assert typ in ("float", "int32_t") and "*" not in names, decl
            out += [n.strip() for n in names.split(",")]
    return out


def prototype(name):
    """[(type, parameter name)] of ``int name(...);``"""
    args = re.search(r"\bint %s\((.*?)\);" % name, HEADER, re.S).group(1)
    out = []
    for a in args.split(","):
        a = " ".join(a.split())
        m = re.match(r"(.*?)(\w+)$", a)
        out.append((m.group(1).strip(), m.group(2)))
    return out


FIELDS = {"ppo": (struct_fields("xt_ppo_cfg"), H.PPO_CFG_FIELDS, H.PPO_CALL),
          "impala": (struct_fields("xt_impala_cfg"), H.IMPALA_CFG_FIELDS, H.IMPALA_CALL)}
POINTERS = {"ppo": ("xt_net_ppo_train", H.PPO_POINTERS), "impala": ("xt_net_impala_train", H.IMPALA_POINTERS)}


def rows_of(entry, what=None, near=None):
    return [r for r in H.MUTATIONS if r["entry"] == entry and (what is None or r["what"] == what) and
            (near is None or r["near"] == near)]


@pytest.mark.parametrize("entry", ["ppo", "impala"])
def test_every_cfg_field_has_a_mutation_row_or_is_exempt(entry):
    parsed, listed, default = FIELDS[entry]
    assert tuple(parsed) == tuple(listed)
    assert set(H.EXEMPT[entry]) == {"shard_rank", "shard_world"}
    assert all(v == "tests/test_gpu_dp*.py" for v in H.EXEMPT[entry].values())
    for f in parsed:
        assert f in default
        if f in H.EXEMPT[entry]:
            assert not rows_of(entry, f)
            continue
        rows = rows_of(entry, f, near=False)
        assert len(rows) == 1, f
        base = H.call_of(rows[0], False)
        assert base[f] != rows[0]["mutated"] and rows[0]["live"], f
        if f in ("rms_decay", "rms_eps"):
            assert base["opt_type"] == "rmsprop", f      # (they act under RMSProp only)
    assert H.call_of(rows_of("impala", "sample_batch_step")[0], False)["sample_batch_step"] == 10
    assert rows_of("impala", "sample_batch_step")[0]["mutated"] == 5


@pytest.mark.parametrize("entry", ["ppo", "impala"])
def test_every_pointer_and_n_and_every_switch_has_a_row(entry):
    name, listed = POINTERS[entry]
    proto = prototype(name)
    ptrs = [n for t, n in proto if "*" in t]
    assert [n for n in ptrs if n not in H.NOT_DATA_POINTERS] == list(listed)
    assert set(H.NOT_DATA_POINTERS) <= set(ptrs)
    for p in listed:
        rows = rows_of(entry, p)
        assert len(rows) == 1 and rows[0]["mutated"] == "B" and H.call_of(rows[0], False)[p] == "A", p
        assert rows[0]["live"] == (p != "loss_acc")      # (the accumulator is written, never read)
    scalars = [n for t, n in proto if "*" not in t and n != "use_graph"]
    assert scalars == (["n"] if entry == "ppo" else ["n", "batch_size"])
    for s in scalars:
        assert len(rows_of(entry, s)) == 1 and rows_of(entry, s)[0]["live"], s
    for sw in (("train_stats", "gauss_fused") if entry == "ppo" else ("impala_stats",)):
        rows = rows_of(entry, sw)
        assert len(rows) == 1 and rows[0]["mutated"] is True and H.call_of(rows[0], False)[sw] is False
    # nothing else is in the table, and no row changes the net itself
    known = set(FIELDS[entry][1]) | set(listed) | set(scalars) | {"train_stats", "gauss_fused", "impala_stats"}
    assert {r["what"] for r in rows_of(entry)} <= known
    assert len(set(H.MUTATION_IDS)) == len(H.MUTATIONS)


def test_mutated_calls_are_calls_the_entries_accept():
    for r in H.MUTATIONS:
        for c in (H.call_of(r, False), H.call_of(r, True)):
            if r["entry"] == "ppo":
                assert 0 < c["batch_size"] <= c["max_batch"] and 0 < c["n"] <= H.PPO_DATA_ROWS
                assert 0 < c["num_sgd_iter"] <= H.PPO_DATA_EPOCHS
                assert c["gauss_fused"] is False or H.NETS[c["net"]]["action_type"] == H.G
            else:
                t = c["sample_batch_step"]
                assert t >= 2 and c["n"] % t == 0 and c["batch_size"] % t == 0 and c["batch_size"] <= c["max_batch"]
                assert 0 < c["n"] <= H.IMPALA_DATA_ROWS and len(H.impala_chunks(c["n"], c["batch_size"])) <= H.IMPALA_DATA_CHUNKS
            assert c["shard_world"] == 0 and c["shard_rank"] == 0


def test_near_collision_rows_collide_under_percent_g_and_differ_as_float32():
    near = [r for r in H.MUTATIONS if r["near"]]
    assert {(r["entry"], r["what"]) for r in near} == {("ppo", "lr"), ("ppo", "clip_ratio"), ("ppo", "max_grad_norm"),
                                                       ("impala", "lr"), ("impala", "gamma")}
    for r in near:
        base = H.call_of(r, False)[r["what"]]
        # live, except where float32 itself makes the two values one: 1 -+ clip_ratio are the same floats for both
        c, c1 = np.float32(H.PPO_CALL["clip_ratio"]), np.float32(H.f32_next(H.PPO_CALL["clip_ratio"]))
        assert np.float32(1) + c == np.float32(1) + c1 and np.float32(1) - c == np.float32(1) - c1
        assert r["live"] == (r["what"] != "clip_ratio"), r["id"]
        # the value the struct holds is the float32; printf promotes it to double, as Python's % does
        b32, m32 = np.float32(base), np.float32(r["mutated"])
        assert b32 != m32 and m32 == np.nextafter(b32, np.float32(np.inf)), r["id"]
        assert "%g" % float(b32) == "%g" % float(m32), r["id"]
        assert float(b32).hex() != float(m32).hex(), r["id"]        # ("%a", what the key prints now)
    assert H.call_of([r for r in near if r["id"] == "impala.lr~"][0], False)["lr_steps"] is None
    # the issue's own two examples
    for v in (2.5e-4, 0.1):
        assert "%g" % float(np.float32(v)) == "%g" % H.f32_next(v)


@pytest.mark.parametrize("rid", H.PPO_LOOP_IDS)
def test_ppo_loop_row_literals_are_the_loop_arithmetic(rid):
    r = H.PPO_LOOP[H.PPO_LOOP_IDS.index(rid)]
    assert r["sizes"] * r["epochs"] == H.ppo_minibatches(r["n"], r["batch"], r["epochs"])
    assert r["steps"] == len(r["sizes"]) * r["epochs"] == -(-r["n"] // r["batch"]) * r["epochs"]
    assert sum(r["sizes"]) == r["n"] and r["max_batch"] == r["batch"] and r["global_batch"] in (0, r["batch"])
    for b in r["sizes"]:
        gb = H.ppo_step_global_batch(r["global_batch"], b, r["batch"])
        assert gb == (b if r["global_batch"] else 0)       # global = local batch: a short minibatch is its own global one
    assert r["n"] <= 33 and r["net"] in H.NETS


@pytest.mark.parametrize("rid", H.IMPALA_LOOP_IDS)
def test_impala_loop_row_literals_are_the_loop_arithmetic(rid):
    r = H.IMPALA_LOOP[H.IMPALA_LOOP_IDS.index(rid)]
    assert r["sizes"] == H.impala_chunks(r["n"], r["batch_size"]) and r["steps"] == len(r["sizes"])
    assert r["n"] % r["T"] == 0 and r["batch_size"] % r["T"] == 0
    assert max(r["sizes"]) <= r["max_batch"]
    assert r["batch_size"] <= r["max_batch"] or r["n"] <= r["max_batch"]      # what the entry accepts


def test_loop_tables_hold_both_sides_of_every_condition():
    p = H.PPO_LOOP
    assert len(set(H.PPO_LOOP_IDS)) == len(p) and len(set(H.IMPALA_LOOP_IDS)) == len(H.IMPALA_LOOP)
    assert any((r["n"], r["batch"], r["epochs"]) == (7, 16, 1) for r in p)
    rel = lambda r: ("lt" if r["n"] < r["batch"] else "eq" if r["n"] == r["batch"] else
                     {0: "2b", 1: "2b+1", -1: "2b-1"}.get(r["n"] - 2 * r["batch"]))
    for cond in ("lt", "eq", "2b", "2b+1", "2b-1"):
        assert {bool(r["global_batch"]) for r in p if rel(r) == cond} >= ({True} if cond == "eq" else {True, False}), cond
    assert any(r["sizes"][-1] == 1 and len(r["sizes"]) > 1 for r in p)
    assert {r["epochs"] for r in p} >= {1, 3}
    short = [r for r in p if r["sizes"][-1] != r["batch"]]
    assert {bool(r["global_batch"]) for r in short} == {True, False}
    assert {r["gauss_fused"] for r in short if r["net"] == "gauss"} == {True, False}
    assert all(r["global_batch"] for r in short if r["net"] == "gauss")
    assert any(r["stats"] and r["global_batch"] and r["sizes"][-1] != r["batch"] for r in p) and any(not r["stats"] for r in p)
    assert {r["net"] for r in p} == {"mlp", "cnn17", "gauss"}
    i = H.IMPALA_LOOP
    assert any(len(r["sizes"]) == 1 and r["n"] < r["batch_size"] <= r["max_batch"] for r in i)
    assert any(r["n"] == r["batch_size"] for r in i)
    assert any(len(r["sizes"]) == 3 and r["sizes"][-1] < r["batch_size"] for r in i)
    assert any(r["batch_size"] > r["max_batch"] and r["n"] <= r["max_batch"] for r in i)
    assert {r["T"] for r in i} == {2, 10}
    for fact in ("lr_steps", "stats"):
        assert {bool(r[fact]) for r in i} == {True, False}, fact
    assert {r["opt"] for r in i} == {"adam", "rmsprop"}
    multi = [r for r in i if len(r["sizes"]) > 1]
    assert {bool(r["lr_steps"]) for r in multi} == {True, False} and {r["opt"] for r in multi} == {"adam", "rmsprop"}


def test_networks_are_the_ones_named_and_the_data_is_seeded():
    for name in H.NETS:
        spec, ospec = H.build_specs(name)
        assert sorted(H.seeded_params(name, ospec)) == sorted(spec.names)
    assert H.build_specs("gauss")[0].action_type == H.G and H.build_specs("impala42")[0].action_dim == 4
    a, b = H.ppo_data("mlp", 20, 2, 10), H.ppo_data("mlp", 20, 2, 11)
    assert all(not np.array_equal(a[k], b[k]) for k in a)
    assert all(np.array_equal(v, H.ppo_data("mlp", 20, 2, 10)[k]) for k, v in a.items())
    a, b = H.impala_data("impala42", 40, 8, 10), H.impala_data("impala42", 40, 8, 11)
    assert all(not np.array_equal(a[k], b[k]) for k in a)


def test_cache_report_is_bound_with_the_headers_signature():
    from xingtian_amd import lib as L
    proto = prototype("xt_net_graph_cache_info")
    assert proto == [("const xt_net*", "net"), ("int32_t*", "out"), ("int32_t", "cap")]
    ctype = {"const xt_net*": ctypes.c_void_p, "int32_t*": ctypes.POINTER(ctypes.c_int32), "int32_t": ctypes.c_int32}
    assert L.SIGNATURES["xt_net_graph_cache_info"] == (ctypes.c_int32, [ctype[t] for t, _ in proto])
    words = re.findall(r"XT_GRAPH_CACHE_(\w+) = (\d+)", HEADER)
    assert [w for w, _ in words] == list(L.GRAPH_CACHE_WORDS) + ["WORDS"]
    assert [int(v) for _, v in words] == list(range(len(L.GRAPH_CACHE_WORDS) + 1))
    # appended under the current ABI number: the last prototype of the header, the version untouched
    assert HEADER.rstrip().rsplit("int xt_net_", 1)[1].startswith("graph_cache_info(")
    assert int(re.search(r"#define XT_ABI_VERSION (\d+)", HEADER).group(1)) == L.ABI_VERSION == 12
    from xingtian_amd.model.hip_net import HipActorCritic
    assert callable(HipActorCritic.graph_cache_info)
