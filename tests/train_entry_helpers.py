"""Case tables of the two whole-update entry points, ``xt_net_ppo_train`` and ``xt_net_impala_train``, shared by
tests/test_cpu_train_entry_coverage.py and tests/test_gpu_train_entry.py (a plain module: numpy only, no fixtures, no
device).

Three tables, every row carrying the facts it is expected to show:

* ``PPO_LOOP`` / ``IMPALA_LOOP``: the minibatch / chunk loops of ``ppo_train_enqueue`` / ``impala_train_enqueue``
  (xingtian_amd/csrc/xt_net.hip) -- ``steps`` and ``sizes`` are literals, the CPU test holds them against a restatement
  of the loop arithmetic (``ppo_minibatches`` ...), the GPU test holds the library against them.
* ``MUTATIONS``: one row per thing that changes the work a train enqueues -- every scalar field of ``xt_ppo_cfg`` /
  ``xt_impala_cfg``, every data pointer, ``n``, the net-level switches -- as ``(entry, what, base, mutated, live)``.
  ``base`` holds the overrides of the entry's default call the row needs (an optimiser under which the field acts, a
  buffer the mutation replaces), ``live`` says that the mutated call must leave other parameters than the base call.
  The near-collision rows change a float to its float32 neighbour: under ``"%g"`` the two print alike.
* ``EXEMPT``: the cfg fields without a row, and what covers them instead.

The float64 references are ``oracle.nets.PpoLearnerOracle`` / ``ImpalaLearnerOracle``, the bars (``BARS``) those of
tests/test_gpu_learner.py's train tests: nothing here is a new tolerance.
"""
from collections import OrderedDict

import numpy as np

from oracle import nets

G = "DiagGaussian"

# tests/test_gpu_learner.py::test_ppo_train_matches_oracle_and_graph_replay_is_bitwise and
# ::test_impala_train_entry_chunks_graph_replay_bitwise_and_device_step_sizes: mean loss 1e-4 * max(1, |ref|), every
# parameter within two lr-sized steps per SGD step, the update 5e-3 relative in the 2-norm (smooth activations only: the
# first Adam steps are sign-like, assert_update_close there)
BARS = dict(loss=1e-4, steps_lr=2.0, delta=5e-3)

# ------------------------------------------------------------------------------------------------ networks
NETS = OrderedDict([
    ("mlp", dict(kind="ppo_mlp", state_dim=(4,), action_dim=2, hidden=(16, 16), act="tanh", share=False,
                 action_type="Categorical")),
    ("cnn17", dict(kind="ppo_cnn", state_dim=(17, 17, 4), action_dim=3, hidden=(32,), act="relu", share=True,
                   action_type="Categorical")),
    ("gauss", dict(kind="ppo_mlp", state_dim=(3,), action_dim=2, hidden=(16,), act="tanh", share=False, action_type=G)),
    ("impala42", dict(kind="impala_cnn_opt", state_dim=(42, 42, 4), action_dim=4, mean=128.0, std=128.0)),
])
SMOOTH = ("mlp", "gauss")       # tanh nets: the update itself is held to BARS["delta"]


def build_specs(name):
    """-> (netspec.NetSpec, oracle spec dict)"""
    from xingtian_amd.model import netspec
    a = NETS[name]
    if a["kind"] == "ppo_mlp":
        spec = netspec.ppo_mlp(a["state_dim"], a["action_dim"], a["hidden"], a["act"], a["share"], a["action_type"])
        ospec = nets.ppo_mlp_spec(a["state_dim"], a["action_dim"], a["hidden"], a["act"], a["share"], a["action_type"])
    elif a["kind"] == "ppo_cnn":
        spec = netspec.ppo_cnn(a["state_dim"], a["action_dim"], a["hidden"], a["act"], a["share"])
        ospec = nets.ppo_cnn_spec(a["state_dim"], a["action_dim"], a["hidden"], a["act"], a["share"])
    else:
        spec = netspec.impala_cnn_opt(a["state_dim"], a["action_dim"], a["mean"], a["std"])
        ospec = nets.impala_cnn_opt_spec(a["state_dim"], a["action_dim"], a["mean"], a["std"])
    return spec, ospec


def seeded_params(name, ospec, seed=0):
    p = nets.init_params(ospec, seed=7 + seed, bias_scale=0.05)
    if "pi_logstd" in p:
        p["pi_logstd"] = (np.random.default_rng(seed).standard_normal(p["pi_logstd"].shape) * 0.3).astype(np.float32)
    return p


def ppo_data(name, n, epochs, seed):
    """a seeded rollout of ``n`` rows and ``epochs`` permutations of it, as tests/net_zoo_helpers.py draws them"""
    a = NETS[name]
    rng = np.random.default_rng(4000 + seed)
    sd, adim = tuple(a["state_dim"]), a["action_dim"]
    if len(sd) == 3:
        obs = rng.integers(0, 256, (n,) + sd).astype(np.uint8)
    else:
        obs = rng.uniform(-1, 1, (n,) + sd).astype(np.float32)
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
    perm = np.stack([rng.permutation(n) for _ in range(epochs)]).astype(np.int32)
    return dict(obs=obs, action=action, old_logp=logp, adv=adv, old_v=old_v, target_v=target_v, perm=perm)


def impala_data(name, n, chunks, seed):
    a = NETS[name]
    rng = np.random.default_rng(5000 + seed)
    adim = a["action_dim"]
    return dict(obs=rng.integers(0, 256, (n,) + tuple(a["state_dim"])).astype(np.uint8),
                bp_logits=rng.standard_normal((n, adim)).astype(np.float32),
                action=rng.integers(0, adim, n).astype(np.int32), done=(rng.random(n) < 0.1).astype(np.uint8),
                reward=rng.choice([-2.0, 0.0, 1.0], n).astype(np.float32),
                lr_steps=(np.float32(6e-4 if seed % 2 else 1e-3) * np.float32(0.5) ** np.arange(chunks)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ the loops, restated
def ppo_minibatches(n, batch, epochs):
    """rows of every SGD step of ``ppo_train_enqueue``, in order: per epoch ceil(n / batch) minibatches, the last short"""
    return [min(batch, n - start) for _ in range(epochs) for start in range(0, n, batch)]


def ppo_step_global_batch(global_batch, rows, batch):
    """the ``global_batch`` the loop hands a minibatch of ``rows``: a short last one keeps the local / global ratio"""
    if global_batch > 0 and rows != batch:
        return global_batch * rows // batch
    return global_batch


def impala_chunks(n, batch_size):
    return [min(batch_size, n - lo) for lo in range(0, n, batch_size)]


# ------------------------------------------------------------------------------------------------ loop tables
def _p(rid, net, n, batch, epochs, gb, sizes, stats=False, gauss_fused=False, seed=0):
    """global_batch ``gb``: 0 or "batch" (= the row's batch: every full minibatch is its own global one, a short one is
    only after the rescaling).  ``sizes``: the minibatches of ONE epoch; ``steps`` = SGD steps of the call."""
    return dict(id=rid, net=net, n=n, batch=batch, epochs=epochs, global_batch=batch if gb == "batch" else 0, sizes=sizes,
                steps=len(sizes) * epochs, stats=stats, gauss_fused=gauss_fused, seed=seed, max_batch=batch)


PPO_LOOP = [
    _p("mlp_n7_b16_e1", "mlp", 7, 16, 1, 0, [7]),                         # n < batch
    _p("mlp_n7_b16_e1_gb", "mlp", 7, 16, 1, "batch", [7]),                # ... its only minibatch is a short one
    _p("mlp_n16_b16_e1_gb", "mlp", 16, 16, 1, "batch", [16]),             # n == batch
    _p("mlp_n32_b16_e3", "mlp", 32, 16, 3, 0, [16, 16]),                  # n == 2 batch
    _p("mlp_n32_b16_e1_gb", "mlp", 32, 16, 1, "batch", [16, 16]),
    _p("mlp_n33_b16_e1_gb", "mlp", 33, 16, 1, "batch", [16, 16, 1]),      # n == 2 batch + 1: a last minibatch of one row
    _p("mlp_n33_b16_e3", "mlp", 33, 16, 3, 0, [16, 16, 1]),
    _p("mlp_n31_b16_e1_gb", "mlp", 31, 16, 1, "batch", [16, 15]),         # n == 2 batch - 1
    _p("mlp_n31_b16_e3", "mlp", 31, 16, 3, 0, [16, 15]),
    _p("cnn17_n15_b7_e1_gb", "cnn17", 15, 7, 1, "batch", [7, 7, 1]),
    _p("cnn17_n13_b7_e3", "cnn17", 13, 7, 3, 0, [7, 6]),
    _p("gauss_n19_b8_e1_gb_fused", "gauss", 19, 8, 1, "batch", [8, 8, 3], gauss_fused=True),
    _p("gauss_n19_b8_e1_gb_plain", "gauss", 19, 8, 1, "batch", [8, 8, 3]),
    _p("mlp_n33_b16_e3_gb_stats", "mlp", 33, 16, 3, "batch", [16, 16, 1], stats=True),
]
PPO_LOOP_IDS = [r["id"] for r in PPO_LOOP]

IMPALA_LR, IMPALA_CLIP = 7e-4, 40.0


def _i(rid, n, batch_size, t, sizes, lr_steps, opt, stats, max_batch=None, seed=0):
    return dict(id=rid, net="impala42", n=n, batch_size=batch_size, T=t, sizes=sizes, steps=len(sizes), lr_steps=lr_steps,
                opt=opt, stats=stats, max_batch=max_batch or batch_size, seed=seed)


IMPALA_LOOP = [
    _i("n20_b40_t10", 20, 40, 10, [20], False, "adam", False),                     # one chunk, n < batch_size
    _i("n20_b20_t10_lr_stats", 20, 20, 10, [20], True, "adam", True),              # n == batch_size
    _i("n50_b20_t10_lr", 50, 20, 10, [20, 20, 10], True, "adam", False),           # three chunks, a short last one
    _i("n50_b20_t10_rms_stats", 50, 20, 10, [20, 20, 10], False, "rmsprop", True),
    _i("n14_b6_t2_rms", 14, 6, 2, [6, 6, 2], False, "rmsprop", False),             # T = 2
    _i("n14_b6_t2_lr_stats", 14, 6, 2, [6, 6, 2], True, "adam", True),
    _i("n20_b60_t10_max20", 20, 60, 10, [20], False, "adam", True, max_batch=20),   # batch_size > maxB, n <= maxB
]
IMPALA_LOOP_IDS = [r["id"] for r in IMPALA_LOOP]


# ------------------------------------------------------------------------------------------------ key mutations
PPO_CFG_FIELDS = ("lr", "beta1", "beta2", "eps", "clip_ratio", "ent_coef", "vf_clip", "critic_coef", "max_grad_norm",
                  "batch_size", "num_sgd_iter", "grad_scale", "global_batch", "shard_rank", "shard_world")
IMPALA_CFG_FIELDS = ("lr", "beta1", "beta2", "eps", "grad_norm_clip", "gamma", "sample_batch_step", "grad_scale",
                     "opt_type", "rms_decay", "rms_eps", "shard_rank", "shard_world")
PPO_POINTERS = ("obs", "perm", "action", "old_logp", "adv", "old_v", "target_v", "loss_acc")
IMPALA_POINTERS = ("obs", "bp_logits", "action", "done", "reward", "lr_steps", "loss_acc")
# pointer parameters of the two prototypes that are not data: the net owns the cache (a rebind empties it: the
# interleaving test), cfg is covered field by field, the stream is where the graph is launched and not what it holds
NOT_DATA_POINTERS = ("net", "cfg", "stream")
# cfg fields without a mutation row: a sharded train needs a gradient exchange, which is data-parallel work
EXEMPT = {
    "ppo": {"shard_rank": "tests/test_gpu_dp*.py", "shard_world": "tests/test_gpu_dp*.py"},
    "impala": {"shard_rank": "tests/test_gpu_dp*.py", "shard_world": "tests/test_gpu_dp*.py"},
}

# the default call of each entry: cfg fields, n, the net's switches, and for every pointer the data set ("A" / "B": two
# seeded rollouts in separate device buffers) it points into.  Six SGD steps (8 + 8 + 4 rows, two epochs) / two chunks.
PPO_CALL = dict(net="mlp", max_batch=8, n=20, lr=2.5e-4, beta1=0.9, beta2=0.999, eps=1e-8, clip_ratio=0.1, ent_coef=0.003,
                vf_clip=5.0, critic_coef=1.0, max_grad_norm=5.0, batch_size=8, num_sgd_iter=2, grad_scale=1.0,
                global_batch=0, shard_rank=0, shard_world=0, train_stats=False, gauss_fused=False,
                obs="A", perm="A", action="A", old_logp="A", adv="A", old_v="A", target_v="A", loss_acc="A")
IMPALA_CALL = dict(net="impala42", max_batch=20, n=40, batch_size=20, lr=7e-4, beta1=0.9, beta2=0.999, eps=1e-8,
                   grad_norm_clip=40.0, gamma=0.99, sample_batch_step=10, grad_scale=1.0, opt_type="adam", rms_decay=0.99,
                   rms_eps=0.1, shard_rank=0, shard_world=0, impala_stats=False,
                   obs="A", bp_logits="A", action="A", done="A", reward="A", lr_steps=None, loss_acc="A")
PPO_DATA_ROWS, PPO_DATA_EPOCHS = 20, 2       # rows / permutations of the data sets "A" and "B"
IMPALA_DATA_ROWS, IMPALA_DATA_CHUNKS = 40, 8


def f32_next(x):
    """the float32 above ``x`` (as a Python float)"""
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def _m(entry, what, mutated, live, base=None, near=False):
    base = dict(base or {})
    default = PPO_CALL if entry == "ppo" else IMPALA_CALL
    assert what in default and all(k in default for k in base), (entry, what, base)
    return dict(id="{}.{}{}".format(entry, what, "~" if near else ""), entry=entry, what=what, base=base, mutated=mutated,
                live=live, near=near)


_RMS = dict(opt_type="rmsprop")
# a norm bound BELOW the gradient norm, so that the clip factor (and its one-ulp change) reaches the update; a larger
# step, so that a one-ulp change of the clipped gradient does not drown in the rounding of params - lr_t * step
_CLIPPED = dict(max_grad_norm=0.05, lr=1e-2)
MUTATIONS = [
    # ---- xt_ppo_cfg
    _m("ppo", "lr", 1e-3, True),
    _m("ppo", "beta1", 0.5, True),
    _m("ppo", "beta2", 0.99, True),
    _m("ppo", "eps", 1e-3, True),
    _m("ppo", "clip_ratio", 0.3, True),
    _m("ppo", "ent_coef", 0.1, True),
    _m("ppo", "vf_clip", 0.05, True),
    _m("ppo", "critic_coef", 0.5, True),
    _m("ppo", "max_grad_norm", 0.01, True, base=_CLIPPED),
    _m("ppo", "batch_size", 5, True),
    _m("ppo", "num_sgd_iter", 1, True),
    _m("ppo", "grad_scale", 0.3, True),            # (not a power of two: Adam is scale-free up to eps and rounding)
    _m("ppo", "global_batch", 24, True),           # (24 = 3 x 8: every mean is a third of the local one)
    # ---- xt_impala_cfg
    _m("impala", "lr", 2e-3, True),
    _m("impala", "beta1", 0.5, True),
    _m("impala", "beta2", 0.99, True),
    _m("impala", "eps", 1e-3, True),
    _m("impala", "grad_norm_clip", 0.5, True),
    _m("impala", "gamma", 0.9, True),
    _m("impala", "sample_batch_step", 5, True),
    _m("impala", "grad_scale", 0.3, True),
    _m("impala", "opt_type", "rmsprop", True),
    _m("impala", "rms_decay", 0.9, True, base=_RMS),
    _m("impala", "rms_eps", 0.01, True, base=_RMS),
    # ---- pointers: another buffer at another address with other contents (loss_acc is written only)
    _m("ppo", "obs", "B", True), _m("ppo", "perm", "B", True), _m("ppo", "action", "B", True),
    _m("ppo", "old_logp", "B", True), _m("ppo", "adv", "B", True),
    _m("ppo", "old_v", "B", True, base=dict(vf_clip=0.05)),      # (old_v acts through the value clip only: at 5.0 it never binds)
    _m("ppo", "target_v", "B", True), _m("ppo", "loss_acc", "B", False),
    _m("impala", "obs", "B", True), _m("impala", "bp_logits", "B", True), _m("impala", "action", "B", True),
    _m("impala", "done", "B", True), _m("impala", "reward", "B", True),
    _m("impala", "lr_steps", "B", True, base=dict(lr_steps="A")), _m("impala", "loss_acc", "B", False),
    # ---- n (fewer rows of the same buffers) and the chunk size
    _m("ppo", "n", 13, True),
    _m("impala", "n", 20, True),
    _m("impala", "batch_size", 10, True),
    # ---- net-level switches
    _m("ppo", "train_stats", True, False),
    _m("impala", "impala_stats", True, False),
    # (the fused head's wave sums may differ from the plain head's in the last bits; on this two-action net they do not)
    _m("ppo", "gauss_fused", True, False, base=dict(net="gauss")),
    # ---- near collisions: the float32 neighbour prints the same six digits
    _m("ppo", "lr", f32_next(2.5e-4), True, near=True),
    # NOT live, and cannot be: the kernels form 1 - c and 1 + c in float32, where c and its neighbour (7.5e-9 apart) round
    # to the same bounds (ulp of 0.9: 6e-8, of 1.1: 1.2e-7) -- the two calls compute the same bits.  The row still holds the
    # key: two captures, or the cache has folded the two values into one graph
    _m("ppo", "clip_ratio", f32_next(0.1), False, near=True),
    _m("ppo", "max_grad_norm", f32_next(0.05), True, base=_CLIPPED, near=True),
    _m("impala", "lr", f32_next(7e-4), True, near=True),
    _m("impala", "gamma", f32_next(0.99), True, near=True),
]
MUTATION_IDS = [r["id"] for r in MUTATIONS]


def call_of(row, mutated):
    """the row's base (or mutated) call: the entry's default, the row's overrides, the mutation"""
    call = dict(PPO_CALL if row["entry"] == "ppo" else IMPALA_CALL, **row["base"])
    if mutated:
        call[row["what"]] = row["mutated"]
    return call


def rel_err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm((got - ref).ravel()) / (np.linalg.norm(ref.ravel()) + 1e-30))
