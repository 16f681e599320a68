"""CPU side of the network zoo (tests/net_zoo_helpers.py): the table covers every value of every plan fact of the update
step, its literal expectations agree with the step's conditions restated in Python, the float64 reference is far from its
own float32 rounding on every row, and ``xt_net_create`` -- host code, no device call -- refuses at construction what no
step could finish."""
import numpy as np
import pytest

import net_zoo_helpers as Z


# ------------------------------------------------------------------------------------------------ the table itself
@pytest.mark.parametrize("rid", Z.ROW_IDS)
def test_row_literals_are_what_the_step_conditions_give(rid):
    row = Z.ROWS[Z.ROW_IDS.index(rid)]
    spec, ospec = Z.build_specs(row)
    assert Z.plan_from_conditions(row, spec) == row["expect"]
    b = row["batch"]
    if row["entry"] == "impala_step":
        assert b[0] in (2, 9) and 1 <= b[1] <= 3
    else:
        assert b in (1, 7, 33)
    assert Z.frames(row) <= 33
    assert set(row["tuning"]) <= set(Z.TUNING_DEFAULTS)
    # every variable of the network has a reference value under the same name (DQN: positionally, dqn_helpers.name_map)
    names = list(Z.nets.init_params(ospec))
    if row["entry"] == "dqn_step":
        assert len(Z.DH.name_map(spec, ospec)) == len(spec.names)
    else:
        assert sorted(names) == sorted(spec.names)


def test_table_covers_every_value_of_every_plan_fact():
    ex = [r["expect"] for r in Z.ROWS]
    assert len(set(Z.ROW_IDS)) == len(Z.ROWS)
    assert {e["head"] for e in ex} == set(Z.HEADS)
    for fact in ("deferred", "mask", "preact", "fuse12", "fuse21", "pad", "dense_conv"):
        assert {e[fact] for e in ex} == {0, 1}, fact
    assert {e["trunks"] for e in ex} == {1, 2}
    assert {e["layers"] for e in ex} >= set(range(1, 10))
    assert {e["tail"] for e in ex} >= {0, 1, 3}
    assert {e["form"] for e in ex} == {0, 2}
    # fuse12 / fuse21 / tail overlap refused WITH the knob on, and the deferral refused by its own knob
    knob = lambda k: [r for r in Z.ROWS if r["tuning"].get(k)]
    assert {r["expect"]["fuse12"] for r in knob("fwd_fuse12")} == {0, 1}
    assert {r["expect"]["fuse21"] for r in knob("bwd_fuse21")} == {0, 1}
    assert {r["expect"]["tail"] for r in knob("tail_overlap")} >= {0, 3}
    assert any(r["tuning"].get("defer_splitk") == 0 and r["expect"]["head"] == "ppo_fused" and not r["expect"]["deferred"]
               for r in Z.ROWS)
    # unshared trunks whose last layers do and do not split K; a swish / gelu last layer on an otherwise fused-head shape
    two = [r["expect"] for r in Z.ROWS if r["expect"]["trunks"] == 2 and r["expect"]["head"] == "ppo_fused"]
    assert {e["deferred"] for e in two} == {0, 1}
    assert any(r["expect"]["preact"] and r["args"]["action_dim"] <= 8 and r["expect"]["head"] == "ppo_plain" for r in Z.ROWS)
    # DiagGaussian: the switch off and on inside the envelope, outside through A and through F with the switch on
    g = [r for r in Z.ROWS if r["args"].get("action_type") == Z.G]
    assert {r["args"]["action_dim"] for r in g} >= {1, 3, 8, 9}
    assert any(r["gauss_fused"] and r["expect"]["head"] == "gauss_plain" and r["args"]["action_dim"] > 8 for r in g)
    assert any(r["gauss_fused"] and r["expect"]["head"] == "gauss_plain" and max(r["args"]["hidden_sizes"]) > 512 for r in g)
    assert any(not r["gauss_fused"] and r["args"]["action_dim"] <= 8 for r in g)
    cat = [r for r in Z.ROWS if r["entry"] == "ppo_step" and r["args"]["action_type"] != Z.G]
    assert {r["args"]["action_dim"] for r in cat} >= {1, 2, 8, 9, 18, 64}
    assert {r["args"]["state_dim"][0] for r in Z.ROWS if r["builder"] == "ppo_mlp"} >= {1, 3, 5, 17, 376}
    assert {r["args"]["state_dim"][0] for r in Z.ROWS if r["builder"] == "ppo_cnn"} >= {84, 42, 15, 64, 9, 3}
    assert {r["args"]["action_dim"] for r in Z.ROWS if r["builder"] == "impala_cnn_opt"} >= {1, 8, 9, 32, 33}
    assert {frozenset(r["args"].items()) for r in Z.ROWS if r["builder"] == "impala_mlp"} and \
        {(r["args"]["hidden_size"], r["args"]["num_layers"]) for r in Z.ROWS if r["builder"] == "impala_mlp"} >= {(36, 1), (128, 3)}
    assert {(r["builder"], r["args"]["dueling"], r["args"]["action_dim"]) for r in Z.ROWS if r["entry"] == "dqn_step"} >= \
        {("dqn_cnn", True, 18), ("dqn_cnn", False, 2), ("dqn_mlp", True, 2), ("dqn_mlp", False, 18)}
    assert {Z.frames(r) for r in Z.ROWS if r["entry"] != "impala_step"} == {1, 7, 33}
    assert any(r["args"].get("input_dtype") == "float32" for r in Z.ROWS)


# ------------------------------------------------------------------------------------------------ the reference alone
@pytest.mark.parametrize("rid", Z.ROW_IDS)
def test_float32_oracle_is_within_a_tenth_of_the_gradient_bar(rid):
    """The same oracle in float32 on the row's own inputs: every gradient tensor within 1e-6 of float64, a tenth of the
    bar the kernels are held to, so a GPU miss points at the kernels and not at the number format.  (Where a row were
    not, its seed or input scale changes, never the bar.)"""
    row = Z.ROWS[Z.ROW_IDS.index(rid)]
    ref = Z.reference(row)
    params = {k: v.copy() for k, v in ref["params"].items()}
    out32 = Z.oracle_step(row, ref["ospec"], params, ref["target_params"], ref["inputs"], np.float32)
    worst, worst_k = 0.0, None
    for k, g64 in ref["out"]["grads"].items():
        if not np.any(g64):
            assert not np.any(out32["grads"][k]), k      # (the hidden 1-wide head of a DQN net without dueling)
            continue
        e = Z.rel_err(out32["grads"][k], g64)
        if e > worst:
            worst, worst_k = e, k
    loss_e = abs(float(out32["loss"]) - float(ref["out"]["loss"])) / max(1.0, abs(float(ref["out"]["loss"])))
    print("f32-oracle {} loss {:.2e} worst-grad {:.2e} ({})".format(rid, loss_e, worst, worst_k))
    assert worst <= Z.ORACLE_F32_GRAD, (rid, worst_k, worst)
    # ... and no relu unit of the reference sits on its kink (net_zoo_helpers.min_relu_preact)
    print("min-relu-z {} {:.2e}".format(rid, ref["out"]["min_relu_z"]))
    assert ref["out"]["min_relu_z"] >= Z.RELU_MARGIN, (rid, ref["out"]["min_relu_z"])
    assert loss_e <= 0.1 * Z.BARS["loss"]


# ------------------------------------------------------------------------------------------------ the construction envelope
def _create(spec, max_batch=8):
    from xingtian_amd import lib
    from xingtian_amd.model import hip_net
    _, _, h = hip_net.create_net(spec, max_batch)
    assert lib.load().xt_net_workspace_bytes(h) > 0
    lib.load().xt_net_destroy(h)


def _unequal_trunks(depths):
    from xingtian_amd.model import netspec
    layers = []
    for trunk, (prefix, sizes) in enumerate(zip(("pi", "v"), depths)):
        layers += netspec._mlp(prefix, 8, sizes, "tanh", trunk)[0]
    return netspec.NetSpec(layers, 2, 64, 2, "pi_latent", "output_value", (64, 2), (0, 0.0, 1.0), (1, 1, 8))


def test_xt_net_create_accepts_nine_layers_and_refuses_ten_naming_the_limit():
    """The gradient table of the step's reduction launch has 12 entries: one per trunk layer, the pi head, the v head and --
    DiagGaussian -- pi_logstd, so nine trunk layers fit with either action type (9 + 3 = 12: pi_logstd is the third
    non-layer entry and lands in the last slot, e[11]).  Ten layers used to fail inside the first update, after its forward
    and head kernels had been enqueued; now no net is built that a step cannot finish."""
    from xingtian_amd import lib
    from xingtian_amd.model import netspec
    assert lib.MAX_TRUNK_LAYERS == 9
    nine = (64, 32, 64, 32, 64, 32)
    _create(netspec.ppo_cnn((15, 15, 4), 4, nine, "tanh", True))
    _create(netspec.ppo_cnn((15, 15, 4), 3, nine, "tanh", True, action_type="DiagGaussian"))
    for spec in (netspec.ppo_cnn((42, 42, 4), 4, (512, 256), "relu", False),             # unshared: 2 x (3 convs + 2 hidden)
                 netspec.ppo_cnn((15, 15, 4), 4, nine + (64,), "tanh", True),
                 netspec.ppo_mlp((4,), 1, (64,) * 5, "tanh", False, action_type="DiagGaussian")):
        with pytest.raises(ValueError, match=r"10 trunk layers.*exceed the limit of 9.*gradient table holds 12"):
            _create(spec)


def test_xt_net_create_refuses_unequal_unshared_trunks_and_empty_layers():
    """``ppo_step`` hands both trunks' last layers to ONE fused head launch and requires them in the same split-K state, and
    both heads read ``feat`` features: unshared trunks are two copies of one stack.  No builder of the YAML surface makes
    anything else; a description that does is refused by name."""
    _create(_unequal_trunks(((64, 64), (64, 64))))
    with pytest.raises(ValueError, match=r"pi and v trunks differ \(2 and 1 layers\).*equal depth"):
        _create(_unequal_trunks(((64, 64), (64,))))
    with pytest.raises(ValueError, match=r"pi and v trunks differ \(2 and 2 layers\).*equal layer geometry"):
        _create(_unequal_trunks(((32, 64), (64, 64))))
    spec = _unequal_trunks(((64,), (64,)))
    spec.layers[1].OH = 0
    with pytest.raises(ValueError, match=r"layer 1 is empty.*at least 1"):
        _create(spec)


@pytest.mark.parametrize("size", [20, 40])
def test_inferred_architectures_that_end_in_an_empty_layer_are_refused_when_the_spec_is_built(size):
    """The reference's inference rule halves a size counter per 5x5/2 layer instead of following the VALID output size: a
    20x20 (40x40) image ends in a 3x3 kernel on a 2x2 map, which TensorFlow refuses as well."""
    from xingtian_amd.model import netspec
    with pytest.raises(ValueError, match=r"3x3 kernel does not fit its 2x2 input.*at least 1x1"):
        netspec.ppo_cnn((size, size, 4), 4, (64,), "relu", True)


def test_python_constructors_surface_the_refusal_as_a_value_error_at_construction():
    from xingtian_amd.model import model_builder, netspec
    from xingtian_amd.model.hip_net import HipActorCritic
    with pytest.raises(ValueError, match="exceed the limit of 9"):
        HipActorCritic(netspec.ppo_cnn((42, 42, 4), 4, (512, 256), "relu", False), max_batch=8)
    cfg = {"action_type": "Categorical", "VF_SHARE_LAYERS": False, "hidden_sizes": [512, 256]}
    info = {"model_name": "PpoCnn", "state_dim": [42, 42, 4], "action_dim": 4, "model_config": cfg, "type": "learner"}
    with pytest.raises(ValueError, match="exceed the limit of 9"):
        model_builder(info)
    with pytest.raises(ValueError, match="does not fit its 2x2 input"):
        model_builder(dict(info, state_dim=[20, 20, 4], model_config=dict(cfg, hidden_sizes=[64])))


def test_step_report_is_host_only_and_sized_by_the_caller():
    """before any step: the capacities and zeros, from a net that was never bound to device memory"""
    import ctypes
    from xingtian_amd import lib
    from xingtian_amd.model import hip_net, netspec
    spec = netspec.ppo_cnn((42, 42, 4), 4, (64,), "swish", False)
    _, _, h = hip_net.create_net(spec, 8)
    try:
        rep = lib.step_report(h)
        assert rep["layers"] == 8 and rep["trunks"] == 2 and rep["finish_form"] == -1 and rep["head_path"] == 0
        assert rep["words"] == len(lib.STEP_REPORT_NET) + 8 * len(lib.STEP_REPORT_LAYER)
        assert rep["partial_floats"] == 512 * 4096 and rep["max_norm_partials"] == 16384
        assert [l["trunk"] for l in rep["layer"]] == [0] * 4 + [1] * 4
        assert all(l["preact"] == 1 and l["ksplit"] == 1 and l["slab_cap"] >= 1 and not l["deferred"] for l in rep["layer"])
        small = (ctypes.c_int32 * 16)()
        assert lib.load().xt_net_last_step_report(h, small, 16) != 0
        assert b"16 words offered" in lib.load().xt_last_error()
    finally:
        lib.load().xt_net_destroy(h)
