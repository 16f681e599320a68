"""CPU side of the knob matrix (tests/knob_matrix_helpers.py): the covering array is deterministic, small, starts at the
defaults, covers every pair of factor values and holds only values ``xt_tuning_set`` accepts; the bases' references keep
the margins their bars need; the prediction of the plan words reduces to the zoo's
literals at the zoo's knobs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import knob_matrix_helpers as K
import net_zoo_helpers as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the array
def test_array_is_deterministic_small_and_covers_every_pair():
    a, b = K.covering_array(), K.covering_array()
    assert a == b and [list(r.items()) for r in a] == [list(r.items()) for r in b]
    assert a == K.array()
    assert len(a) <= K.MAX_ROWS == 32
    assert all(list(r) == list(K.FACTORS) and all(r[n] in K.FACTORS[n] for n in r) for r in a)
    assert not K.uncovered_pairs(a)
    # ... and no row is spare: without any one of them a pair is lost (row 0, the defaults, is the reference row)
    for drop in range(1, len(a)):
        assert K.uncovered_pairs(a[:drop] + a[drop + 1:]) or drop <= len(K.pinned_rows()), drop
    # another seed gives another array of the same kind
    c = K.covering_array(seed=K.ARRAY_SEED + 1)
    assert c != a and not K.uncovered_pairs(c) and len(c) <= K.MAX_ROWS
    print("rows", len(a), "pairs", len(K.all_pairs()))


def test_row_zero_is_what_a_fresh_process_reports():
    """every xt_tuning field is a factor, in the struct's order, and row 0 holds the library's own defaults"""
    code = "import json; from xingtian_amd import lib; print(json.dumps(lib.get_tuning()))"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, check=True, stdout=subprocess.PIPE).stdout
    fresh = json.loads(out.decode().strip().splitlines()[-1])
    from xingtian_amd import lib
    assert K.TUNING_NAMES == [n for n, _ in lib.Tuning._fields_] == list(fresh)
    row0 = K.array()[0]
    assert {n: row0[n] for n in K.TUNING_NAMES} == fresh
    assert row0["fwd_fuse12_flat"] == 1 and row0["bwd_dense_lean"] == 1      # both switches are on by default
    assert all(v[0] == K.DEFAULTS[n] and len(set(v)) == len(v) >= 2 for n, v in K.FACTORS.items())
    # the multi-valued factors hold the values their descriptions document
    doc = dict(wgrad_rows={4, 0, 1, 2}, tail_overlap={0, 1, 2, 3}, bwd_fuse21={0, 1, 2}, dense_wgrad_x6={1, 0, 2},
               reduce_z_lanes={8, 16, 1}, conv1_waves={8, 4}, fwd_fuse12={0, 4096}, bwd_fit_slots={768, 0},
               reduce_deep_lanes={128, 0})
    assert all(set(K.FACTORS[n]) == v for n, v in doc.items())


def test_pinned_rows():
    """rows 1..8: one of the eight knobs the fused conv1 -> conv2 launch pins is off, the other seven hold; rows 9 and 10:
    bwd_fuse21 taken behind the fused launch and behind the flat first layer"""
    a = K.array()
    for i, fix in enumerate(K.pinned_rows(), 1):
        assert all(a[i][n] == v for n, v in fix.items()), i
    s255, s33 = K.build(K.B255)[0], K.build(K.CNN33)[0]
    w33, w255 = K.expected_words(K.CNN33, s33, a[9]), K.expected_words(K.B255, s255, a[9])
    assert w33["conv12"] and w33["bwd_fuse21"] and w255["conv12"] and w255["bwd_fuse21"]
    w33, w255 = K.expected_words(K.CNN33, s33, a[10]), K.expected_words(K.B255, s255, a[10])
    assert not w33["bwd_fuse21"] and w255["bwd_fuse21"] and not w255["conv12"] and w255["mask_valid"][0]
    # rows 11 and 12: both one-launch conv1 -> conv2 forwards run with tail_overlap 3 / 2 honoured on the bases that train
    imp = K.BASES["impala84_a4_t9x3"]["row"]
    for i, tail in ((11, 3), (12, 2)):
        w33, wimp = K.expected_words(K.CNN33, s33, a[i]), K.expected_words(imp, K.build(imp)[0], a[i])
        assert w33["conv12"] and w33["tail_overlap"] == tail and wimp["fwd_fuse12"] and wimp["tail_overlap"] == tail
    for i, e in enumerate(K.ENVELOPE_KNOBS, 1):
        off = [n for n in K.ENVELOPE_KNOBS if a[i][n] != K.DEFAULTS[n]]
        assert off == [e], (i, off)
        assert not K.envelope_knobs_hold(a[i])
        assert K.envelope_knobs_hold(dict(a[i], **{e: K.DEFAULTS[e]}))
    assert K.envelope_knobs_hold(a[0])


def test_every_row_is_accepted_by_xt_tuning_set_and_the_previous_values_come_back():
    from xingtian_amd import lib
    before = lib.get_tuning()
    lean = lib.set_bwd_dense_lean(True)
    try:
        for i, r in enumerate(K.array()):
            old = lib.set_tuning(**K.tuning_of(r))
            try:
                assert lib.get_tuning() == K.tuning_of(r), i
                assert lib.set_bwd_dense_lean(bool(r["bwd_dense_lean"])) in (True, False)
            finally:
                lib.set_tuning(**old)
            assert lib.get_tuning() == before, i
    finally:
        lib.set_bwd_dense_lean(lean)
    assert lib.set_bwd_dense_lean(lean) == lean


def test_block_count_targets_change_a_split_count_at_the_matrix_shapes():
    for knob, (what, at_default, at_second) in K.split_count_changes().items():
        print("{}: {} -> {} ({})".format(knob, at_default, at_second, what))
        assert at_default != at_second, knob
    assert set(K.split_count_changes()) == {"fwd_split_target", "wgrad_split_target", "direct_waves", "direct_max_waves",
                                            "direct_tile64_tiles"}


# ------------------------------------------------------------------------------------------------ the bases
@pytest.mark.parametrize("bid", list(K.BASES))
def test_seed_conditions_of_the_base(bid):
    """Every base is held to the zoo's bars, and its reference keeps the margins those bars need.  For the three zoo shapes:
    the float32 oracle within ORACLE_F32_GRAD (a tenth of the gradient bar) of the float64 one on every gradient tensor, no
    relu unit within RELU_MARGIN of its kink.  The 255-frame base, where no seed of 1..64 reaches either, is held to its own
    figures (``knob_matrix_helpers.B255``): float32 rounding below half the gradient bar, relu margin four times the rounding
    estimate."""
    base = K.BASES[bid]
    row = base["row"]
    ref = Z.reference(row)
    out32 = Z.oracle_step(row, ref["ospec"], {k: v.copy() for k, v in ref["params"].items()}, None, ref["inputs"], np.float32)
    worst = max(Z.rel_err(out32["grads"][k], g) for k, g in ref["out"]["grads"].items())
    loss_e = abs(float(out32["loss"]) - float(ref["out"]["loss"])) / max(1.0, abs(float(ref["out"]["loss"])))
    margin = ref["out"]["min_relu_z"]
    print("base {} f32-oracle loss {:.2e} worst-grad {:.2e} min-relu-z {:.2e}".format(bid, loss_e, worst, margin))
    assert worst <= base["f32_grad"] and margin >= base["relu_margin"], (bid, worst, margin)
    assert loss_e <= 0.1 * base["bars"]["loss"]
    assert base["bars"] == Z.BARS
    if bid == "cnn84_h256_a4_b255":
        assert base["f32_grad"] < 0.5 * Z.BARS["grad"] and 0.95 * base["f32_grad"] <= worst      # (no looser than measured)
        assert base["relu_margin"] == 4 * 5e-8 and not (base["second"] or base["train"])
    else:
        assert (base["f32_grad"], base["relu_margin"]) == (Z.ORACLE_F32_GRAD, Z.RELU_MARGIN)
    if bid in Z.ROW_IDS:      # the zoo's shape: its own row, or that row under another seed (knob_matrix_helpers.CNN33)
        zoo = Z.ROWS[Z.ROW_IDS.index(bid)]
        assert row is zoo or {k: v for k, v in row.items() if k not in ("id", "seed")} == \
            {k: v for k, v in zoo.items() if k not in ("id", "seed")}


def test_bases_are_the_issue_shapes():
    assert list(K.BASES) == ["cnn84_h512_a4_b33", "impala84_a4_t9x3", "mlp376_h256x3_a8_b33", "cnn84_h256_a4_b255"]
    r = K.B255
    assert r["args"]["hidden_sizes"] == (256,) and r["args"]["action_dim"] == 4 and r["args"]["vf_share"] and Z.frames(r) == 255
    spec = K.build(r)[0]
    l1 = spec.layers[1]
    # 255 frames: the first batch with >= 200 blocks of 128 conv2 input positions, the threshold of bwd_fuse21 = 1
    assert Z._cdiv(255 * (l1.H // 2) * (l1.W // 2), 128) == 200 > Z._cdiv(254 * (l1.H // 2) * (l1.W // 2), 128)
    assert [b for b, v in K.BASES.items() if v["second"]] == ["cnn84_h512_a4_b33", "mlp376_h256x3_a8_b33"]
    assert {b: v["train"] for b, v in K.BASES.items() if v["train"]} == {"cnn84_h512_a4_b33": "ppo", "impala84_a4_t9x3": "impala"}


@pytest.mark.parametrize("bid", [b for b, v in K.BASES.items() if v["second"]])
def test_second_step_reference_keeps_the_relu_margin(bid):
    """the float64 oracle's own second step, from its own step-1 parameters: no relu unit on its kink"""
    row = K.BASES[bid]["row"]
    ref, first = Z.reference(row), K.first_step_state(row)
    for k, p in ref["out"]["params"].items():      # (the shared first step is the reference's)
        assert np.array_equal(first["params"][k], p), k
    _, out2 = K.ppo_oracle_at(row, ref["ospec"], first["params"], ref["inputs"], steps_before=1, m=first["m"], v=first["v"])
    print("second-step min-relu-z {} {:.2e}".format(bid, out2["min_relu_z"]))
    assert out2["min_relu_z"] >= Z.RELU_MARGIN
    moved = max(Z.rel_err(out2["grads"][k], g) for k, g in ref["out"]["grads"].items())
    assert moved > 100 * Z.BARS["grad"], moved      # one update moves the gradients far beyond the bar: stale weights would show


# ------------------------------------------------------------------------------------------------ the prediction
def test_extended_prediction_gives_every_zoo_row_its_literals():
    for row in Z.ROWS:
        spec, _ = Z.build_specs(row)
        assert K.zoo_facts(row, spec) == row["expect"], row["id"]
        assert K.zoo_facts(row, spec) == Z.plan_from_conditions(row, spec), row["id"]


def test_prediction_over_the_matrix():
    """every (base, row) has a prediction; the interactions the conditions name show up in it"""
    a = K.array()
    seen = dict(open=0, conv12=0, fuse21=0, fuse12=0, tail=set(), form=set(), nodefer=0, mask0=0)
    for bid, base in K.BASES.items():
        row = base["row"]
        spec, b = K.build(row)[0], Z.frames(row)
        for ri, knobs in enumerate(a):
            w = K.expected_words(row, spec, knobs)
            is_open = K.conv12_envelope_open(spec, b, knobs)
            assert not w["conv12"] or (is_open and knobs["fwd_fuse12_flat"])
            assert not is_open or (K.envelope_knobs_hold(knobs) and w["mask_valid"][0] == 1)
            assert not w["bwd_fuse21"] or (w["mask_valid"][0] and knobs["bwd_fuse21"])
            assert not (w["tail_overlap"] and knobs["finalize_ticket"]) and not (w["tail_overlap"] and spec.n_trunks == 2)
            assert w["finish_form"] in ((0,), (1,), (2,), (2, 3)) and (3 not in w["finish_form"] or (
                knobs["tail_fused"] and not w["tail_overlap"]))
            assert all(d == int(k > 1) or not d for d, k in zip(w["deferred"], w["ksplit"]))
            assert knobs["defer_splitk"] or row["entry"] == "impala_step" or not any(w["deferred"])
            if ri == 0:
                assert K.zoo_facts(dict(row, tuning={}), spec) == row["expect"]
            seen["open"] += is_open
            seen["conv12"] += w["conv12"]
            seen["fuse21"] += w["bwd_fuse21"]
            seen["fuse12"] += w["fwd_fuse12"]
            seen["tail"].add(w["tail_overlap"])
            seen["form"].add(w["finish_form"])
            seen["nodefer"] += int(not any(w["deferred"]))
            seen["mask0"] += int(not w["mask_valid"][0])
    print({k: (sorted(v) if isinstance(v, set) else v) for k, v in seen.items()})
    # the fused conv12 launch: open at the defaults on 255 frames, closed on 33 (conv2 splits K there) until the split
    # target stops that, closed on every edge row
    s255, s33 = K.build(K.B255)[0], K.build(K.BASES["cnn84_h512_a4_b33"]["row"])[0]
    assert K.conv12_envelope_open(s255, 255, a[0]) and not K.conv12_envelope_open(s33, 33, a[0])
    assert K.conv12_envelope_open(s33, 33, dict(a[0], fwd_split_target=16))
    assert not any(K.conv12_envelope_open(s255, 255, a[i]) for i in range(1, 1 + len(K.ENVELOPE_KNOBS)))
    assert seen["tail"] == {0, 1, 2, 3} and seen["fuse21"] and seen["fuse12"] and seen["conv12"] and seen["nodefer"] and seen["mask0"]
    assert {(1,), (2,)} <= seen["form"]
