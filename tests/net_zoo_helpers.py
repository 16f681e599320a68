"""The network zoo: one row per configurable network shape, shared by tests/test_cpu_net_zoo_coverage.py and
tests/test_gpu_net_zoo.py (a plain module, no fixtures).

A row names a ``netspec`` builder and its arguments, the entry point that runs one update on it, the batch, tuning
overrides and the PLAN FACTS the step must report for it (``lib.step_report``): literal values, written down from the
conditions in xingtian_amd/csrc/xt_net.hip.  ``plan_from_conditions`` restates those conditions in Python (and the few
launcher rules they lean on: the split-K cut of ``launch_fwd``, the geometry tests of the first-layer kernels, the
``bwd_fuse21`` branch of ``plan_bwd_layer``); the CPU test holds every row's literals against it, the GPU test holds the
library's report against the literals.

The float64 reference of every entry point is the one its existing whole-step test uses (``oracle.nets`` learners,
``tests/dqn_helpers.py``), and so are the bars (``BARS``): nothing here is a new tolerance.
"""
from collections import OrderedDict

import numpy as np

from oracle import nets
import dqn_helpers as DH

# ------------------------------------------------------------------------------------------------ bars (existing ones)
# tests/test_gpu_learner.py::test_ppo_step_loss_and_grads_vs_oracle, ::test_impala_step_vs_oracle,
# ::test_keras_impala_models_fit_vs_oracle (loss, update) and tests/test_gpu_dqn.py::test_net_dqn_step_against_float64:
# loss 1e-4 * max(1, |loss|); every gradient tensor 1e-5 relative in the 2-norm; PPO gradient norm 1e-4 relative; the
# update by tests/test_gpu_learner.py::assert_update_close
BARS = dict(loss=1e-4, grad=1e-5, gnorm=1e-4)
ORACLE_F32_GRAD = 1e-6      # the float32 oracle against the float64 one: a tenth of the gradient bar

PPO_CFG = dict(LR=2.5e-4, LOSS_CLIPPING=0.1, ENTROPY_LOSS=0.003, VF_CLIP=5.0, CRITIC_LOSS_COEF=1.0, MAX_GRAD_NORM=5.0,
               NUM_SGD_ITER=1)
IMPALA_LR, IMPALA_CLIP = 5e-4, 40.0
KERAS_LR, KERAS_ENT = 3e-4, 0.01
DQN_GAMMA = 0.99
PREACT = ("swish", "gelu")
TUNING_DEFAULTS = dict(defer_splitk=1, bwd_fuse21=0, fwd_fuse12=0, tail_overlap=0)

# head classes of the report's HEAD_PATH word (include/xt_mi355x.h: XT_HEAD_PATH_* in the low 4 bits, XT_NET_HEAD_*)
HEADS = ("ppo_fused", "ppo_plain", "gauss_fused", "gauss_plain", "impala_fused", "impala_loss", "none")


def head_class(word):
    word &= 0xffffffff
    if word == 0:
        return "none"
    if word == 0x10000:
        return "ppo_plain"
    if word == 0x20000:
        return "gauss_plain"
    return {1: "ppo_fused", 2: "impala_fused", 3: "impala_loss", 4: "gauss_fused"}[word & 0xf]


# ------------------------------------------------------------------------------------------------ the table
def _row(rid, builder, args, entry, batch, expect, tuning=None, gauss_fused=False, seed=0, obs_scale=1.0):
    return dict(id=rid, builder=builder, args=args, entry=entry, batch=batch, expect=expect, tuning=tuning or {},
                gauss_fused=gauss_fused, seed=seed, obs_scale=obs_scale)


def _x(head, layers, trunks=1, deferred=0, mask=0, preact=0, fuse12=0, fuse21=0, tail=0, form=2, pad=0, dense_conv=0):
    """the plan facts of a row: head class, layer / trunk counts, whether the trunks' last layers leave split-K partials to
    the head, whether the first layer's sign mask is valid, whether any layer keeps its pre-activation, fuse12 / fuse21
    taken, the tail-overlap bits honoured, the form of the gradient-reduction launch; and two facts of the description
    itself: channel padding of the image, a whole-image conv run as Dense"""
    return dict(head=head, layers=layers, trunks=trunks, deferred=deferred, mask=mask, preact=preact, fuse12=fuse12,
                fuse21=fuse21, tail=tail, form=form, pad=pad, dense_conv=dense_conv)


def _cnn(sd, a, hidden, act="relu", share=True, dtype="uint8", action_type="Categorical"):
    return dict(state_dim=sd, action_dim=a, hidden_sizes=hidden, act=act, vf_share=share, input_dtype=dtype,
                action_type=action_type)


def _mlp(width, a, hidden, act="tanh", share=False, action_type="Categorical"):
    return dict(state_dim=(width,), action_dim=a, hidden_sizes=hidden, act=act, vf_share=share, action_type=action_type)


G = "DiagGaussian"
ROWS = [
    # ---- PpoCnn: table and inferred images, hidden sizes, action dimensions
    _row("cnn84_h512_a4_b7", "ppo_cnn", _cnn((84, 84, 4), 4, (512,)), "ppo_step", 7, _x("ppo_fused", 4, deferred=1, mask=1)),
    _row("cnn84_h512_a4_b33", "ppo_cnn", _cnn((84, 84, 4), 4, (512,)), "ppo_step", 33, _x("ppo_fused", 4, deferred=1, mask=1)),
    _row("cnn42_h64_a2_b33", "ppo_cnn", _cnn((42, 42, 4), 2, (64,)), "ppo_step", 33, _x("ppo_fused", 4, deferred=1)),
    _row("cnn15_h36_a8_b7", "ppo_cnn", _cnn((15, 15, 4), 8, (36,)), "ppo_step", 7, _x("ppo_fused", 4, deferred=1)),
    _row("cnn64_h100_a9_b1", "ppo_cnn", _cnn((64, 64, 4), 9, (100,)), "ppo_step", 1, _x("ppo_plain", 5)),
    _row("cnn17_h4_a1_b7", "ppo_cnn", _cnn((17, 17, 4), 1, (4,)), "ppo_step", 7, _x("ppo_fused", 3, deferred=1)),
    _row("cnn9_h512_a18_b33", "ppo_cnn", _cnn((9, 9, 4), 18, (512,)), "ppo_step", 33, _x("ppo_plain", 3, dense_conv=1)),
    _row("cnn3_h516_a4_b7", "ppo_cnn", _cnn((3, 3, 4), 4, (516,)), "ppo_step", 7, _x("ppo_plain", 2)),
    _row("cnn84c3_h64_a64_b7", "ppo_cnn", _cnn((84, 84, 3), 64, (64,)), "ppo_step", 7, _x("ppo_plain", 4, mask=1, pad=1)),
    _row("cnn42f32_h64_a2_b7", "ppo_cnn", _cnn((42, 42, 4), 2, (64,), dtype="float32"), "ppo_step", 7,
         _x("ppo_fused", 4, deferred=1)),
    _row("cnn42_h512_256_a4_b7", "ppo_cnn", _cnn((42, 42, 4), 4, (512, 256)), "ppo_step", 7, _x("ppo_fused", 5, deferred=1)),
    _row("cnn42_8layers_a4_b7", "ppo_cnn", _cnn((42, 42, 4), 4, (64, 64, 64, 64, 64), act="tanh"), "ppo_step", 7,
         _x("ppo_fused", 8)),
    _row("cnn64_7layers_a2_b1", "ppo_cnn", _cnn((64, 64, 4), 2, (64, 36, 64)), "ppo_step", 1, _x("ppo_fused", 7)),
    _row("cnn15_9layers_a4_b7", "ppo_cnn", _cnn((15, 15, 4), 4, (64, 32, 64, 32, 64, 32), act="tanh"), "ppo_step", 7,
         _x("ppo_fused", 9)),
    # nine layers AND pi_logstd: the twelfth and last entry of the gradient table
    _row("cnn15_9layers_gauss_a3_b7", "ppo_cnn", _cnn((15, 15, 4), 3, (64, 32, 64, 32, 64, 32), act="tanh", action_type=G),
         "ppo_step", 7, _x("gauss_plain", 9)),
    # ---- both sharing modes: unshared trunks whose last layers split K (Dense 3136 -> 64) and do not (64 -> 64)
    _row("cnn42_unshared_h64_a6_b7", "ppo_cnn", _cnn((42, 42, 4), 6, (64,), act="tanh", share=False), "ppo_step", 7,
         _x("ppo_fused", 8, trunks=2, deferred=1)),
    _row("cnn15_unshared_h36_a9_b7", "ppo_cnn", _cnn((15, 15, 4), 9, (36,), share=False), "ppo_step", 7,
         _x("ppo_plain", 8, trunks=2)),
    # ---- DiagGaussian: inside the envelope (switch off / on), outside through A, outside through F
    _row("cnn42_gauss_a1_off_b7", "ppo_cnn", _cnn((42, 42, 4), 1, (64,), act="tanh", action_type=G), "ppo_step", 7,
         _x("gauss_plain", 4)),
    _row("cnn42_gauss_a3_on_b7", "ppo_cnn", _cnn((42, 42, 4), 3, (64,), act="tanh", action_type=G), "ppo_step", 7,
         _x("gauss_fused", 4, deferred=1), gauss_fused=True),
    _row("mlp17_gauss_a8_on_b33", "ppo_mlp", _mlp(17, 8, (64, 64), action_type=G), "ppo_step", 33,
         _x("gauss_fused", 4, trunks=2), gauss_fused=True),
    _row("mlp17_gauss_a8_off_b33", "ppo_mlp", _mlp(17, 8, (64, 64), action_type=G), "ppo_step", 33,
         _x("gauss_plain", 4, trunks=2)),
    _row("mlp5_gauss_a9_on_b7", "ppo_mlp", _mlp(5, 9, (32,), share=True, action_type=G), "ppo_step", 7,
         _x("gauss_plain", 1), gauss_fused=True),
    _row("mlp3_gauss_a3_h516_on_b7", "ppo_mlp", _mlp(3, 3, (516,), share=True, action_type=G), "ppo_step", 7,
         _x("gauss_plain", 1), gauss_fused=True),
    _row("mlp3_gauss_a1_b1", "ppo_mlp", _mlp(3, 1, (64, 64), action_type=G), "ppo_step", 1, _x("gauss_plain", 4, trunks=2)),
    # ---- PpoMlp: state widths, depths, one-layer trunks in both sharing modes
    _row("mlp1_h64_64_a2_b7", "ppo_mlp", _mlp(1, 2, (64, 64)), "ppo_step", 7, _x("ppo_fused", 4, trunks=2)),
    _row("mlp376_h256x3_a8_b33", "ppo_mlp", _mlp(376, 8, (256, 256, 256)), "ppo_step", 33,
         _x("ppo_fused", 6, trunks=2, deferred=1)),
    _row("mlp376_h256x3_shared_a2_b1", "ppo_mlp", _mlp(376, 2, (256, 256, 256), share=True), "ppo_step", 1,
         _x("ppo_fused", 3, deferred=1)),
    _row("mlp5_h32_a18_b33", "ppo_mlp", _mlp(5, 18, (32,)), "ppo_step", 33, _x("ppo_plain", 2, trunks=2)),
    _row("mlp17_h64_shared_a4_b7", "ppo_mlp", _mlp(17, 4, (64,), share=True), "ppo_step", 7, _x("ppo_fused", 1)),
    _row("mlp17_h64_unshared_a4_b7", "ppo_mlp", _mlp(17, 4, (64,)), "ppo_step", 7, _x("ppo_fused", 2, trunks=2)),
    # ---- activations: relu and tanh above; swish / gelu keep their pre-activation, on the last layer of a fused-head shape too
    _row("cnn42_swish_h64_a4_b7", "ppo_cnn", _cnn((42, 42, 4), 4, (64,), act="swish"), "ppo_step", 7,
         _x("ppo_plain", 4, preact=1)),
    _row("mlp5_gelu_h64_64_a2_b33", "ppo_mlp", _mlp(5, 2, (64, 64), act="gelu"), "ppo_step", 33,
         _x("ppo_plain", 4, trunks=2, preact=1)),
    _row("mlp5_relu_h64_64_a2_b33", "ppo_mlp", _mlp(5, 2, (64, 64), act="relu", share=True), "ppo_step", 33,
         _x("ppo_fused", 2)),
    # ---- ImpalaCnnOpt: 42 / 84, fused and unfused heads, the one-launch conv1 + conv2 forward offered and not
    _row("impala42_a1_t2x3", "impala_cnn_opt", dict(state_dim=(42, 42, 4), action_dim=1, mean=128.0, std=128.0),
         "impala_step", (2, 3), _x("impala_fused", 3, deferred=1, dense_conv=1)),
    _row("impala42_a8_t9x2", "impala_cnn_opt", dict(state_dim=(42, 42, 4), action_dim=8, mean=128.0, std=128.0),
         "impala_step", (9, 2), _x("impala_fused", 3, deferred=1, dense_conv=1)),
    _row("impala42_a9_t9x1", "impala_cnn_opt", dict(state_dim=(42, 42, 4), action_dim=9, mean=128.0, std=128.0),
         "impala_step", (9, 1), _x("impala_loss", 3, dense_conv=1)),
    _row("impala84_a32_t2x1", "impala_cnn_opt", dict(state_dim=(84, 84, 4), action_dim=32, mean=0.0, std=255.0),
         "impala_step", (2, 1), _x("impala_loss", 3, dense_conv=1)),
    _row("impala84_a33_t9x3", "impala_cnn_opt", dict(state_dim=(84, 84, 4), action_dim=33, mean=0.0, std=255.0),
         "impala_step", (9, 3), _x("impala_loss", 3, dense_conv=1)),
    _row("impala84_a4_t9x3", "impala_cnn_opt", dict(state_dim=(84, 84, 4), action_dim=4, mean=0.0, std=255.0),
         "impala_step", (9, 3), _x("impala_fused", 3, deferred=1, dense_conv=1)),
    # ---- Keras IMPALA pair
    _row("keras_cnn84_a5_b7", "impala_cnn", dict(state_dim=(84, 84, 4), action_dim=5), "keras_impala_step", 7,
         _x("none", 4, mask=1, form=0)),
    _row("keras_cnn36_a5_b33", "impala_cnn", dict(state_dim=(36, 36, 4), action_dim=5), "keras_impala_step", 33,
         _x("none", 4, form=0, dense_conv=1)),      # (36 -> 8 -> 3: the 3x3 conv covers its whole input; no flat conv1, no mask)
    _row("keras_mlp6_h36_l1_a3_b33", "impala_mlp", dict(state_dim=(6,), action_dim=3, hidden_size=36, num_layers=1),
         "keras_impala_step", 33, _x("none", 1, form=0)),
    _row("keras_mlp6_h128_l3_a3_b7", "impala_mlp", dict(state_dim=(6,), action_dim=3, hidden_size=128, num_layers=3),
         "keras_impala_step", 7, _x("none", 3, form=0)),
    # ---- DQN pair, with and without the dueling stream
    _row("dqn_cnn84_a18_dueling_b7", "dqn_cnn", dict(state_dim=(84, 84, 4), action_dim=18, dueling=True), "dqn_step", 7,
         _x("none", 4, mask=1, form=0)),
    _row("dqn_cnn84_a2_plain_b1", "dqn_cnn", dict(state_dim=(84, 84, 4), action_dim=2, dueling=False), "dqn_step", 1,
         _x("none", 4, mask=1, form=0)),
    _row("dqn_mlp4_a2_dueling_b33", "dqn_mlp", dict(state_dim=(4,), action_dim=2, hidden_size=32, num_layers=1, dueling=True),
         "dqn_step", 33, _x("none", 1, form=0)),
    _row("dqn_mlp4_a18_plain_b7", "dqn_mlp", dict(state_dim=(4,), action_dim=18, hidden_size=128, num_layers=3, dueling=False),
         "dqn_step", 7, _x("none", 3, form=0)),
    # ---- tuning: the non-default values of the four net-level knobs on two of the shapes above (and fuse12 refused on 42)
    _row("cnn84_h512_a4_b33_nodefer", "ppo_cnn", _cnn((84, 84, 4), 4, (512,)), "ppo_step", 33,
         _x("ppo_fused", 4, mask=1), tuning=dict(defer_splitk=0)),
    _row("cnn84_h512_a4_b33_fuse21", "ppo_cnn", _cnn((84, 84, 4), 4, (512,)), "ppo_step", 33,
         _x("ppo_fused", 4, deferred=1, mask=1, fuse21=1), tuning=dict(bwd_fuse21=2)),
    _row("cnn42_h64_a2_b33_fuse21_refused", "ppo_cnn", _cnn((42, 42, 4), 2, (64,)), "ppo_step", 33,
         _x("ppo_fused", 4, deferred=1), tuning=dict(bwd_fuse21=2)),
    _row("cnn84_h512_a4_b33_tail3", "ppo_cnn", _cnn((84, 84, 4), 4, (512,)), "ppo_step", 33,
         _x("ppo_fused", 4, deferred=1, mask=1, tail=3), tuning=dict(tail_overlap=3)),
    _row("mlp17_h64_shared_a4_b7_tail3", "ppo_mlp", _mlp(17, 4, (64,), share=True), "ppo_step", 7, _x("ppo_fused", 1),
         tuning=dict(tail_overlap=3)),       # one layer: the overlap is refused
    _row("impala84_a4_t9x3_fuse12", "impala_cnn_opt", dict(state_dim=(84, 84, 4), action_dim=4, mean=0.0, std=255.0),
         "impala_step", (9, 3), _x("impala_fused", 3, deferred=1, fuse12=1, dense_conv=1), tuning=dict(fwd_fuse12=4096)),
    _row("impala84_a4_t9x3_fuse12_small", "impala_cnn_opt", dict(state_dim=(84, 84, 4), action_dim=4, mean=0.0, std=255.0),
         "impala_step", (9, 3), _x("impala_fused", 3, deferred=1, dense_conv=1), tuning=dict(fwd_fuse12=16)),      # 27 frames > 16
    _row("impala42_a8_t9x2_fuse12_refused", "impala_cnn_opt", dict(state_dim=(42, 42, 4), action_dim=8, mean=128.0, std=128.0),
         "impala_step", (9, 2), _x("impala_fused", 3, deferred=1, dense_conv=1), tuning=dict(fwd_fuse12=4096)),
    _row("impala84_a4_t9x3_tail1", "impala_cnn_opt", dict(state_dim=(84, 84, 4), action_dim=4, mean=0.0, std=255.0),
         "impala_step", (9, 3), _x("impala_fused", 3, deferred=1, tail=1, dense_conv=1), tuning=dict(tail_overlap=1)),
]
ROW_IDS = [r["id"] for r in ROWS]
# Seeds of the rows whose float32 ORACLE missed 1e-6 against float64 at seed 0 (1.1e-6 .. 7.2e-6, all on bias gradients or
# one-column head kernels: a float32 sum of thousands of signed terms that cancel): chosen from 1..8 by that CPU
# comparison alone (tests/test_cpu_net_zoo_coverage.py; the first seed from 1 up that passes both of its checks), never by
# a figure a kernel gave.  The bars did not move.
SEEDS = {"cnn84_h512_a4_b33": 7, "cnn84_h512_a4_b33_nodefer": 7, "cnn84_h512_a4_b33_fuse21": 7, "cnn84_h512_a4_b33_tail3": 7,
         "cnn42_h64_a2_b33": 11, "cnn42_h64_a2_b33_fuse21_refused": 11, "cnn15_h36_a8_b7": 2, "cnn64_h100_a9_b1": 6,
         "cnn3_h516_a4_b7": 1, "cnn42_h512_256_a4_b7": 6, "cnn42_8layers_a4_b7": 7, "cnn64_7layers_a2_b1": 2,
         "cnn15_9layers_a4_b7": 5, "cnn15_9layers_gauss_a3_b7": 2, "cnn15_unshared_h36_a9_b7": 3, "cnn42_unshared_h64_a6_b7": 8,
         "mlp17_h64_shared_a4_b7": 1, "mlp17_h64_shared_a4_b7_tail3": 1, "cnn42_swish_h64_a4_b7": 8,
         "impala84_a4_t9x3": 4, "impala84_a4_t9x3_fuse12": 4, "impala84_a4_t9x3_fuse12_small": 4, "impala84_a4_t9x3_tail1": 4,
         # ... and of the rows whose float64 reference had a relu unit on its kink (min_relu_preact below)
         "impala84_a33_t9x3": 37, "cnn84_h512_a4_b7": 3, "keras_cnn84_a5_b7": 3}
for _r in ROWS:
    _r["seed"] = SEEDS.get(_r["id"], 0)


def frames(row):
    b = row["batch"]
    return b[0] * b[1] if isinstance(b, tuple) else b


# ------------------------------------------------------------------------------------------------ specs
def build_specs(row):
    """-> (netspec.NetSpec, oracle spec dict)"""
    from xingtian_amd.model import netspec
    a, k = row["args"], row["builder"]
    if k == "ppo_cnn":
        spec = netspec.ppo_cnn(a["state_dim"], a["action_dim"], a["hidden_sizes"], a["act"], a["vf_share"], a["input_dtype"],
                               a["action_type"])
        ospec = nets.ppo_cnn_spec(a["state_dim"], a["action_dim"], a["hidden_sizes"], a["act"], a["vf_share"])
        if a["action_type"] == G:
            ospec["action_type"] = G
    elif k == "ppo_mlp":
        spec = netspec.ppo_mlp(a["state_dim"], a["action_dim"], a["hidden_sizes"], a["act"], a["vf_share"], a["action_type"])
        ospec = nets.ppo_mlp_spec(a["state_dim"], a["action_dim"], a["hidden_sizes"], a["act"], a["vf_share"], a["action_type"])
    elif k == "impala_cnn_opt":
        spec = netspec.impala_cnn_opt(a["state_dim"], a["action_dim"], a["mean"], a["std"])
        ospec = nets.impala_cnn_opt_spec(a["state_dim"], a["action_dim"], a["mean"], a["std"])
    elif k == "impala_cnn":
        spec, ospec = netspec.impala_cnn(a["state_dim"], a["action_dim"]), nets.impala_cnn_spec(a["state_dim"], a["action_dim"])
    elif k == "impala_mlp":
        spec = netspec.impala_mlp(a["state_dim"], a["action_dim"], a["hidden_size"], a["num_layers"])
        ospec = nets.impala_mlp_spec(a["state_dim"], a["action_dim"], a["hidden_size"], a["num_layers"])
    elif k == "dqn_cnn":
        spec, ospec = netspec.dqn_cnn(a["state_dim"], a["action_dim"], a["dueling"]), DH.oracle_spec("cnn", a["state_dim"], a["action_dim"])
    elif k == "dqn_mlp":
        spec = netspec.dqn_mlp(a["state_dim"], a["action_dim"], a["hidden_size"], a["num_layers"], a["dueling"])
        ospec = DH.oracle_spec("mlp", a["state_dim"], a["action_dim"], a["hidden_size"], a["num_layers"])
    else:
        raise KeyError(k)
    return spec, ospec


def is_image(row):
    return len(row["args"]["state_dim"]) == 3


def is_u8(row):
    return is_image(row) and row["args"].get("input_dtype", "uint8") == "uint8"


# ------------------------------------------------------------------------------------------------ inputs and the oracle
def make_inputs(row):
    """seeded host inputs of the row's one step (numpy), as its entry point's existing whole-step test draws them"""
    rng = np.random.default_rng(1000 + row["seed"])
    a, entry = row["args"], row["entry"]
    sd, adim, b = tuple(a["state_dim"]), a["action_dim"], frames(row)
    n = b if entry == "impala_step" else b + 5

    def states(count):
        if is_u8(row):
            return rng.integers(0, 256, (count,) + sd).astype(np.uint8)
        return (rng.uniform(-1, 1, (count,) + sd) * row["obs_scale"]).astype(np.float32)

    if entry == "ppo_step":
        obs = states(n)
        if a["action_type"] == G:
            action = rng.standard_normal((n, adim)).astype(np.float32)
            logp = (-np.abs(rng.standard_normal((n, 1))) - 0.5).astype(np.float32)
        else:
            action = rng.integers(0, adim, n).astype(np.int32)
            lg = rng.standard_normal((n, adim))
            lsm = lg - np.log(np.exp(lg).sum(-1, keepdims=True))
            logp = np.take_along_axis(lsm, action[:, None].astype(np.int64), 1).astype(np.float32)
        adv = rng.standard_normal((n, 1))
        old_v = rng.standard_normal((n, 1)).astype(np.float32)
        target_v = old_v.astype(np.float64) + rng.standard_normal((n, 1))
        return dict(obs=obs, action=action, logp=logp, adv=adv, old_v=old_v, target_v=target_v,
                    idx=rng.permutation(n)[:b].astype(np.int32))
    if entry == "impala_step":
        return dict(obs=states(n), bp=rng.standard_normal((n, adim)).astype(np.float32),
                    action=rng.integers(0, adim, n).astype(np.int32), done=rng.random(n) < 0.05,
                    reward=rng.choice([-2.0, 0.0, 1.0, 3.0], n).astype(np.float32))
    if entry == "keras_impala_step":
        return dict(obs=states(n), adv=rng.standard_normal((n, 1)).astype(np.float32),
                    onehot=np.eye(adim, dtype=np.float32)[rng.integers(0, adim, n)],
                    target_v=rng.standard_normal((n, 1)).astype(np.float32), idx=rng.permutation(n)[:b].astype(np.int32))
    if entry == "dqn_step":
        return dict(cur=states(n), nxt=states(n), action=rng.integers(0, adim, n).astype(np.int32),
                    reward=rng.standard_normal(n), done=(rng.random(n) < 0.3).astype(np.uint8),
                    slots=rng.permutation(n)[:b].astype(np.int32))
    raise KeyError(entry)


def seeded_params(row, ospec):
    """-> (online parameters, target parameters or None) under the oracle's names"""
    if row["entry"] == "dqn_step":
        d = row["args"]["dueling"]
        return DH.seeded_params(ospec, 1 + row["seed"], d), DH.seeded_params(ospec, 2 + row["seed"], d)
    p = nets.init_params(ospec, seed=7 + row["seed"], bias_scale=0.05)
    if "pi_logstd" in p:
        p["pi_logstd"] = (np.random.default_rng(row["seed"]).standard_normal(p["pi_logstd"].shape) * 0.3).astype(np.float32)
    return p, None


RELU_MARGIN = 2.5e-7      # see min_relu_preact


def min_relu_preact(ac):
    """smallest |pre-activation| over the relu / leaky_relu layers of the oracle net's last forward (inf: none).  A float32
    sum of K terms of size t carries a rounding error of about sqrt(K) * 2^-24 * t: 5e-8 for a first layer (K = 256,
    t ~ 0.05), less behind it.  A unit that the float64 reference puts closer to zero than that can come out on the other
    side of the kink, and at a few frames ONE flipped unit moves a bias gradient by 1e-3 (measured: |z| = 2.1e-8 in conv1
    of the 27-frame ImpalaCnnOpt A = 33 row at seed 0 -> first-layer bias gradient 1.6e-3 off on the device, every other
    figure of that row inside its bar).  Rows keep ``RELU_MARGIN`` = 2.5e-7, five times that error, clear of it; where a
    row did not, its seed changed (``SEEDS``)."""
    m = np.inf
    for trunk, tc in zip(ac.spec["trunks"], ac.cache):
        for lay, (_, _, z) in zip(trunk, tc):
            if lay.act in ("relu", "leaky_relu"):
                m = min(m, float(np.abs(z).min()))
    return m


def oracle_step(row, ospec, params, target_params, inp, dtype=np.float64):
    """one update of the row in ``dtype`` -> dict(loss, grads, params (after the update), gnorm or None, lr, min_relu_z)"""
    entry, b = row["entry"], frames(row)
    if entry == "ppo_step":
        cfg = dict(PPO_CFG, BATCH_SIZE=b)
        orc = nets.PpoLearnerOracle(ospec, params, cfg, dtype)
        i = inp["idx"]
        f32 = lambda x: x[i].astype(np.float32)
        out = orc.step(inp["obs"][i], inp["action"][i], f32(inp["logp"]), f32(inp["adv"]), f32(inp["old_v"]),
                       f32(inp["target_v"]), apply=True)
        return dict(loss=out["loss"], grads=out["grads"], params=orc.net.params, gnorm=out["gnorm"], lr=cfg["LR"],
                    min_relu_z=min_relu_preact(orc.net))
    if entry == "impala_step":
        cfg = dict(LR=IMPALA_LR, grad_norm_clip=IMPALA_CLIP, sample_batch_step=row["batch"][0], BATCH_SIZE=b)
        orc = nets.ImpalaLearnerOracle(ospec, params, cfg, dtype)
        out = orc.step(inp["obs"], inp["bp"], inp["action"], inp["done"], inp["reward"], apply=True)
        return dict(loss=out["loss"], grads=out["grads"], params=orc.net.params, gnorm=None, lr=IMPALA_LR,
                    min_relu_z=min_relu_preact(orc.net))
    if entry == "keras_impala_step":
        orc = nets.KerasImpalaOracle(ospec, params, lr=KERAS_LR, ent_coef=KERAS_ENT, dtype=dtype)
        i = inp["idx"]
        out = orc.step(inp["obs"][i], inp["adv"][i].astype(dtype), inp["onehot"][i].astype(dtype),
                       inp["target_v"][i].astype(dtype), apply=True)
        return dict(loss=out["loss"], grads=out["grads"], params=orc.net.params, gnorm=None, lr=KERAS_LR,
                    min_relu_z=min_relu_preact(orc.net))
    if entry == "dqn_step":
        a = row["args"]
        orc = DH.DqnOracle(ospec, params, target_params, a["dueling"], False, DQN_GAMMA, lr=KERAS_LR, dtype=dtype)
        s = inp["slots"]
        out = orc.step(inp["cur"][s], inp["nxt"][s], inp["action"][s], inp["reward"][s], inp["done"][s], apply=False)
        return dict(loss=out["loss"], grads=out["grads"], params=None, gnorm=None, lr=KERAS_LR,
                    min_relu_z=min_relu_preact(orc.net))
    raise KeyError(entry)


_REF = {}


def reference(row):
    """the float64 reference of the row, computed once per process and shared (callers must not change it)"""
    if row["id"] not in _REF:
        spec, ospec = build_specs(row)
        params, tparams = seeded_params(row, ospec)
        inp = make_inputs(row)
        init = OrderedDict((k, np.array(v, copy=True)) for k, v in params.items())
        _REF[row["id"]] = dict(spec=spec, ospec=ospec, params=init, target_params=tparams, inputs=inp,
                               out=oracle_step(row, ospec, params, tparams, inp, np.float64))
    return _REF[row["id"]]


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm((got - ref).ravel()) / (np.linalg.norm(ref.ravel()) + 1e-30))


# ------------------------------------------------------------------------------------------------ the step's conditions
def _cdiv(a, b):
    return -(-a // b)


def fwd_split(lay, b, target=256):
    """xt_net.hip ``fwd_split``: the split-K factor the step ASKS the forward launch of ``lay`` for"""
    m, n, k = b * lay.OH * lay.OW, lay.N, lay.K
    tiles = _cdiv(m, 128) * _cdiv(n, 32) if n <= 32 else _cdiv(m, 64) * _cdiv(n, 64)
    ksteps = _cdiv(k, 32)
    if tiles >= 128 or ksteps < 4:
        return 1
    return max(1, min(target // tiles, ksteps // 2, 16))


def _padded(lay):
    return lay.PT != 0 or lay.PL != 0 or (lay.OH - 1) * lay.S + lay.KH > lay.H or (lay.OW - 1) * lay.S + lay.KW > lay.W


def launch_ksplit(lay, b, split, identity_input=True, has_idx=False):
    """the split-K factor ``launch_fwd`` (xt_igemm.hip) cuts a float32-input layer into when asked for ``split``, at the
    default knobs: the register-direct kernel (xt_direct.hip ``launch_fwd_direct``) takes single-column-tile shapes with a
    long reduction and slices by its own wave target, everything else is ``pick_ksplit_chunk``"""
    m, n, k = b * lay.OH * lay.OW, lay.N, lay.K
    tiled_first = n <= 32 and k >= 256 and not _padded(lay)
    direct = (not tiled_first and not has_idx and identity_input and lay.C % 16 == 0 and k % 32 == 0 and n % 32 == 0 and
              n % 64 != 0 and k >= 256)
    if direct:
        nsteps, tiles = k // 32, _cdiv(m, 32) * (n // 32)
        slices = max(1, min(_cdiv(1536, tiles), nsteps // 2))
        ks = max(1, min(_cdiv(slices, min(slices, 8)), max(split, 1)))
        return _cdiv(nsteps, _cdiv(nsteps, ks))
    steps = _cdiv(k, 32)
    return _cdiv(steps, _cdiv(steps, max(split, 1)))


def _conv1_flat_mask(lay, xf, b):
    """the flattened uint8 first-layer forward (xt_conv1.hip ``launch_conv1_fwd_bf16x3``) is the one kernel that writes
    the relu sign mask: 8x8 VALID on 4 (padded) channels into 32 relu filters, plain x / std scaling, 256-position ranges
    that touch at most two frame stacks"""
    if not (xf[0] and lay.C == 4 and lay.KH == 8 and lay.KW == 8 and lay.N == 32 and lay.PT == 0 and lay.PL == 0 and
            lay.act == "relu" and abs(xf[1]) < 1e-4 and not _padded(lay)):
        return False
    if (lay.H * lay.W * 4) % 16 or lay.H * lay.W * 4 > 64 * 1024 or (lay.W * 4) % 8 or (lay.S * 4) % 8:
        return False
    total = b * lay.OH * lay.OW
    two = _cdiv(total, 512) >= 200
    return (511 if two else 255) // (lay.OH * lay.OW) + 2 <= (3 if two else 2)


def plan_from_conditions(row, spec):
    """the row's plan facts from the step's conditions (see the module docstring) -> the dict ``_x`` builds"""
    t = dict(TUNING_DEFAULTS, **row["tuning"])
    lays, b, entry = spec.layers, frames(row), row["entry"]
    xf = spec.input_xform
    begin = [min(i for i, l in enumerate(lays) if l.trunk == tr) for tr in range(spec.n_trunks)]
    end = [max(i for i, l in enumerate(lays) if l.trunk == tr) + 1 for tr in range(spec.n_trunks)]
    pre = [l.act in PREACT for l in lays]
    gauss = spec.action_type == G
    lp, lv = end[0] - 1, end[-1] - 1
    inside = spec.action_dim <= 8 and spec.feat <= 512
    if entry == "ppo_step":
        fused = (not gauss or row["gauss_fused"]) and inside and not pre[lp] and not pre[lv]
        offered = fused and t["defer_splitk"] != 0
        head = ("gauss_" if gauss else "ppo_") + ("fused" if fused else "plain")
    elif entry == "impala_step":
        fused = spec.n_trunks == 1 and inside and row["batch"][0] <= 256 and not pre[lp]
        offered = fused
        head = "impala_fused" if fused else "impala_loss"
    else:
        fused = offered = False
        head = "none"
    # the last layer of every trunk: partials left for the head when the launch really splits
    ks = []
    for tr in range(spec.n_trunks):
        lay, first = lays[end[tr] - 1], end[tr] - 1 == begin[tr]
        u8_first = first and xf[0]
        k = 1
        if offered and not pre[end[tr] - 1] and not u8_first:
            k = launch_ksplit(lay, b, fwd_split(lay, b), identity_input=True, has_idx=first and entry == "ppo_step")
        ks.append(k)
    deferred = int(offered and all(k > 1 for k in ks))
    assert len(set(k > 1 for k in ks)) == 1, "the trunks end in different split-K states"
    mask = int(lays[0].N == 32 and lays[0].act == "relu" and _conv1_flat_mask(lays[0], xf, b))
    # fwd_fuse12: ImpalaCnnOpt's 8x8/4 SAME conv1 into 16 filters + 4x4 conv2 into 32, both without mask / pre-activation
    l0 = lays[0]
    fuse12 = 0
    if t["fwd_fuse12"] > 0 and b <= t["fwd_fuse12"] and end[0] - begin[0] >= 3 and not pre[0] and not pre[1] and \
            not (l0.N == 32 and l0.act == "relu"):      # (a first layer with a sign-mask region is not offered)
        l1 = lays[1]
        fuse12 = int(bool(xf[0]) and l0.C == 4 and l0.N == 16 and l0.KH == 8 and l0.KW == 8 and l0.S == 4 and l0.W % 2 == 0 and
                      0 <= xf[1] <= 255 and float(xf[1]).is_integer() and l0.OH * l0.OW <= 14 * 32 and l1.C == 16 and
                      l1.N == 32 and l1.KH == 4 and l1.KW == 4 and l1.H == l0.OH and l1.W == l0.OW and l1.OH * l1.OW <= 128)
    # bwd_fuse21: one trunk, PpoCnn's relu 8x8/4 conv1 (its mask valid) under the all-classes 4x4/2 conv2 backward
    fuse21 = 0
    if t["bwd_fuse21"] != 0 and spec.n_trunks == 1 and len(lays) >= 2 and mask:
        l1 = lays[1]
        n_dg = _cdiv(b * (l1.H // 2) * (l1.W // 2), 128)
        classes = (l1.S == 2 and l1.KH == 4 and l1.KW == 4 and l1.H % 2 == 0 and l1.W % 2 == 0 and l1.C == 32 and
                   l1.N == 32 and not _padded(l1))
        fuse21 = int(classes and l0.OH == l1.H and l0.OW == l1.W and (l0.S * 4) % 16 == 0 and
                     (t["bwd_fuse21"] == 2 or n_dg >= 200) and 512 - n_dg >= 8 * _cdiv(l1.K, 128))
    tail = 0
    if entry in ("ppo_step", "impala_step") and spec.n_trunks == 1 and len(lays) >= 2 and lays[0].param_off == 0:
        tail = t["tail_overlap"] & 3
    form = 2 if entry in ("ppo_step", "impala_step") else 0
    sd = row["args"]["state_dim"]
    pad = int(len(sd) == 3 and sd[2] % 4 != 0)
    dense_conv = int(any(len(l.kernel_shape) == 4 and l.KH == 1 and l.H == 1 and l.kernel_shape[0] > 1 for l in lays))
    return _x(head, len(lays), spec.n_trunks, deferred, mask, int(any(pre)), fuse12, fuse21, tail, form, pad, dense_conv)


def report_facts(rep, spec):
    """``lib.step_report`` -> the same dict (the description facts ``pad`` / ``dense_conv`` are not the report's: None)"""
    lay = rep["layer"]
    ends = [max(i for i, l in enumerate(lay) if l["trunk"] == tr) for tr in range(rep["trunks"])]
    deferred = [lay[e]["deferred"] for e in ends]
    assert len(set(deferred)) == 1, ("the trunks ended in different split-K states", deferred)
    return _x(head_class(rep["head_path"]), rep["layers"], rep["trunks"], deferred[0], lay[0]["mask_valid"],
              int(any(l["preact"] for l in lay)), rep["fwd_fuse12"], rep["bwd_fuse21"], rep["tail_overlap"],
              rep["finish_form"], None, None)
