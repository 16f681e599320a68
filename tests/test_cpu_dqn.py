"""DQN without a GPU: registry and defaults, the network descriptions, the ring sampler against ``deque`` +
``random.sample``, the algorithm's host logic against the executed reference (tests/golden/alg_dqn.npz), the CPU replica's
``predict`` and the C ABI of the three new entries."""
import collections
import json
import os
import random
import re

import numpy as np
import pytest

import dqn_helpers as H  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _module_constants_restored():
    """import_config overrides the modules' constants for the rest of the process: put them back"""
    from xingtian_amd.algorithm.dqn import dqn
    from xingtian_amd.model.dqn import dqn_cnn, dqn_mlp
    saved = [(m, {k: v for k, v in vars(m).items() if k.isupper()}) for m in (dqn, dqn_cnn, dqn_mlp)]
    yield
    for m, consts in saved:
        vars(m).update(consts)


@pytest.fixture(scope="module")
def configs(golden_dir):
    with open(os.path.join(golden_dir, "dqn_configs.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "alg_dqn.npz"))


# ------------------------------------------------------------------------------------------------ registry
def test_registry_resolves_dqn_and_defaults_equal_the_reference(configs):
    import xingtian_amd.algorithm  # noqa: F401
    import xingtian_amd.model  # noqa: F401
    from xingtian_amd.algorithm.dqn import default_config as alg_defaults
    from xingtian_amd.algorithm.dqn.dqn import DQN
    from xingtian_amd.model.dqn import default_config as model_defaults
    from xingtian_amd.model.dqn.dqn_cnn import DqnCnn
    from xingtian_amd.model.dqn.dqn_mlp import DqnMlp
    from xingtian_amd.register import Registers
    assert Registers.algorithm["DQN"] is DQN
    assert Registers.model["DqnCnn"] is DqnCnn and Registers.model["DqnMlp"] is DqnMlp
    upper = lambda mod: {k: getattr(mod, k) for k in dir(mod) if k.isupper()}
    assert upper(alg_defaults) == configs["defaults"]["algorithm/dqn"]
    assert upper(model_defaults) == configs["defaults"]["model/dqn"]


def test_every_dqn_example_yields_a_spec_and_pong_is_refused_with_the_documented_message(configs):
    from xingtian_amd.model.dqn.dqn_cnn import PONG_MESSAGE, dqn_spec
    seen = collections.Counter()
    for path, cfg in configs["yamls"].items():
        assert cfg["alg_para"]["alg_name"] == "DQN", path
        actor = cfg["model_para"]["actor"]
        seen[actor["model_name"]] += 1
        if actor["model_name"] == "DqnCnnPong":
            with pytest.raises(NotImplementedError) as info:
                dqn_spec(actor)
            assert str(info.value) == PONG_MESSAGE and "int8" in PONG_MESSAGE
            continue
        spec = dqn_spec(actor)
        assert spec.action_dim == actor["action_dim"] and spec.n_trunks == 1 and spec.hidden_v
        assert spec.feat == (256 if actor["model_name"] == "DqnCnn" else 128)
    assert seen["DqnCnn"] >= 6 and seen["DqnMlp"] == 1 and seen["DqnCnnPong"] == 1
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        assert "DqnCnnPong" in f.read()


# ------------------------------------------------------------------------------------------------ spec
@pytest.mark.parametrize("dueling", [False, True])
def test_dqn_specs_names_shapes_offsets(dueling):
    from xingtian_amd.model import netspec
    s = netspec.dqn_cnn((84, 84, 4), 6, dueling)
    want = [("conv2d/kernel", (8, 8, 4, 32)), ("conv2d/bias", (32,)), ("conv2d_1/kernel", (4, 4, 32, 64)),
            ("conv2d_1/bias", (64,)), ("conv2d_2/kernel", (3, 3, 64, 64)), ("conv2d_2/bias", (64,)),
            ("dense/kernel", (3136, 256)), ("dense/bias", (256,)), ("dense_1/kernel", (256, 6)), ("dense_1/bias", (6,))]
    if dueling:
        want += [("dense_2/kernel", (256, 1)), ("dense_2/bias", (1,))]
    assert [(k, tuple(v[1])) for k, v in s.names.items()] == want
    off = 0
    for name, shape in want[:8:2]:                      # trunk blocks: kernel then bias, 16-byte aligned blocks
        assert s.names[name][0] == off and off % 4 == 0
        k, n = int(np.prod(shape[:-1])), shape[-1]
        assert s.names[name.replace("kernel", "bias")][0] == off + k * n
        off = (off + (k + 1) * n + 3) & ~3
    assert s.pi_off == off == s.names["dense_1/kernel"][0] and s.names["dense_1/bias"][0] == off + 256 * 6
    assert s.v_off == ((off + 256 * 6 + 6 + 3) & ~3) and s.n_flat == ((s.v_off + 257 + 3) & ~3)
    assert s.hidden_v == (not dueling)
    assert s.n_params == sum(int(np.prod(sh)) for _, sh in want)
    assert s.input_xform == (1, 0.0, 255.0) and s.action_type == "Categorical"
    if dueling:
        assert s.names["dense_2/kernel"][0] == s.v_off and s.names["dense_2/bias"][0] == s.v_off + 256
    else:                                                # the hidden head overlaps no named tensor
        spans = [s.var_extent(k) for k in s.names]
        assert all(o + n <= s.v_off for o, n in spans)
    m = netspec.dqn_mlp((4,), 2, 32, 2, dueling)
    mwant = ["dense/kernel", "dense/bias", "dense_1/kernel", "dense_1/bias", "dense_2/kernel", "dense_2/bias"]
    mwant += ["dense_3/kernel", "dense_3/bias"] if dueling else []
    assert list(m.names) == mwant and m.names["dense_2/kernel"] == (m.pi_off, (32, 2)) and m.feat == 32
    assert m.names["dense/kernel"][1] == (4, 32) and m.names["dense_1/kernel"][1] == (32, 32)


def test_hidden_head_is_absent_from_weights_and_keras_segments():
    from xingtian_amd.model import netspec
    from xingtian_amd.model.cpu_net import CpuActorCritic, initial_weights
    from xingtian_amd.model.hip_net import HipActorCritic
    s = netspec.dqn_mlp((4,), 2, 32, 1, False)
    assert set(initial_weights(s, 0)) == set(s.names) == {"dense/kernel", "dense/bias", "dense_1/kernel", "dense_1/bias"}
    net = CpuActorCritic(s, seed=3)
    assert set(net.get_weights()) == set(s.names)
    assert not net.params[s.v_off:s.v_off + s.feat + 1].any()          # zero-initialised
    # the segments xt_adam_keras walks are built from spec.names alone (HipActorCritic._keras_segments)
    import inspect
    src = inspect.getsource(HipActorCritic._keras_segments)
    assert "for name in self.spec.names" in src and "v_off" not in src
    segs = [s.var_extent(k) for k in s.names]
    assert all(not (o < s.v_off + s.feat + 1 and s.v_off < o + n) for o, n in segs)


def test_existing_impala_specs_are_unchanged_by_the_hidden_head_keyword():
    """offsets and names of the Keras IMPALA specs, as they were before ``hidden_v`` existed (written out here)"""
    from xingtian_amd.model import netspec
    s = netspec.impala_cnn((84, 84, 4), 4)
    assert [(k, v[0]) for k, v in s.names.items()] == [
        ("conv2d/kernel", 0), ("conv2d/bias", 8192), ("conv2d_1/kernel", 8224), ("conv2d_1/bias", 40992),
        ("conv2d_2/kernel", 41056), ("conv2d_2/bias", 77920), ("dense/kernel", 77984), ("dense/bias", 880800),
        ("output_actions/kernel", 881056), ("output_actions/bias", 882080), ("output_value/kernel", 882084),
        ("output_value/bias", 882340)]
    assert (s.pi_off, s.v_off, s.n_flat, s.n_params, s.hidden_v) == (881056, 882084, 882344, 882341, False)
    m = netspec.impala_mlp((4,), 2, 128, 1)
    assert [(k, v[0]) for k, v in m.names.items()] == [
        ("dense/kernel", 0), ("dense/bias", 512), ("output_actions/kernel", 640), ("output_actions/bias", 896),
        ("output_value/kernel", 900), ("output_value/bias", 1028)]
    assert (m.pi_off, m.v_off, m.n_flat, m.hidden_v) == (640, 900, 1032, False)
    d = netspec.dqn_cnn((84, 84, 4), 4, True)           # same trunk and heads, other names
    assert [v for v in d.names.values()] == [v for v in s.names.values()] and d.n_flat == s.n_flat


# ------------------------------------------------------------------------------------------------ sampler
@pytest.mark.parametrize("capacity", [5, 50])
def test_ring_sampler_draws_what_random_sample_draws_from_the_deque(capacity):
    from xingtian_amd.algorithm.dqn.dqn import DeviceReplay
    ring, dq, tag = DeviceReplay(capacity), collections.deque(maxlen=capacity), 0
    assert ring.size() == 0 and ring.cur_state is None                  # allocated at the first add
    sizes = (capacity - 2, 2, 1, capacity + 7, 3) if capacity == 5 else (20, 20, 10, 20, capacity + 13, 7)
    seen = set()
    for n in sizes:                                                     # below, equal to, beyond the capacity; one long message
        tags = np.arange(tag, tag + n)
        tag += n
        ring.add(np.stack([tags, tags * 2], 1).astype(np.float32), np.stack([tags + 0.5, tags], 1).astype(np.float32),
                 tags % 3, tags * 0.1, tags % 2 == 0)
        dq.extend((float(t), int(t % 3), float(t * 0.1), float(t + 0.5), bool(t % 2 == 0)) for t in tags)
        assert ring.size() == len(dq)
        seen.add(len(dq) < capacity)
        for k in sorted({1, len(dq), min(len(dq), 32)}):                # (32 > size: DQN.train asks for min(size, 32))
            random.seed(1000 + n + k)
            want = random.sample(dq, k)
            random.seed(1000 + n + k)
            slots = ring.sample(k)
            got = [(float(ring.cur_state[s, 0]), int(ring.action[s]), float(ring.reward[s]), float(ring.next_state[s, 0]),
                    bool(ring.done[s])) for s in slots]
            assert got == want and all(0 <= s < capacity for s in slots)
    assert seen == {True, False}


# ------------------------------------------------------------------------------------------------ host logic
class _ReplayModel(object):
    """stands in for the model: returns the Q values the reference's recording model returned, in call order, and
    checks that it is asked about the same rows"""
    instances = []

    def __init__(self, model_info):
        self.role = "actor" if not _ReplayModel.instances else "target"
        _ReplayModel.instances.append(self)
        self.queue, self.trains, self.weights = [], [], {"phase": np.float64(len(_ReplayModel.instances) - 1)}

    def predict(self, state):
        tags, q = self.queue.pop(0)
        assert np.array_equal(np.asarray(state)[:, 0], tags), (self.role, np.asarray(state)[:, 0], tags)
        return q.copy()

    def train(self, state, label):
        self.trains.append((np.array(state), np.array(label)))
        return 0.5 + len(self.trains)

    def get_weights(self):
        return dict(self.weights)

    def set_weights(self, w):
        self.weights = dict(w)
        self.sets = getattr(self, "sets", 0) + 1


@pytest.mark.parametrize("mode", ["plain", "double"])
def test_algorithm_host_logic_against_the_executed_reference(golden, mode):
    from xingtian_amd.algorithm import alg_builder
    from xingtian_amd.register import Registers
    _ReplayModel.instances = []
    Registers.model._by_name["_ReplayModel"] = _ReplayModel
    try:
        cfg = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1,
               "BUFFER_SIZE": int(golden["cfg_BUFFER_SIZE"]), "BATCH_SIZE": int(golden["cfg_BATCH_SIZE"]),
               "TARGET_UPDATE_FREQ": int(golden["cfg_TARGET_UPDATE_FREQ"])}
        if mode == "double":
            cfg["double_dqn"] = True
        alg = alg_builder("DQN", {"actor": {"model_name": "_ReplayModel", "state_dim": [3], "action_dim": 3}}, cfg)
    finally:
        del Registers.model._by_name["_ReplayModel"]
    actor, target = alg.actor, alg.target_actor
    assert not alg.device_step and alg.buff.size() == 0 and alg.train_ready(0)
    gamma = float(golden["gamma"])
    random.seed(int(golden["seed"]))
    j = 0
    for step in golden[mode + "_script"]:
        if step >= 0:
            msg = {k: golden["%s_msg%d_%s" % (mode, step, k)] for k in ("cur_state", "next_state", "action", "reward", "done")}
            alg.prepare_data(msg)
            continue
        g = lambda k: golden["%s_train%d_%s" % (mode, j, k)]
        assert alg.buff.size() == int(g("size"))
        actor.queue.append((g("tags"), g("y_pred")))
        target.queue.append((g("next_tags"), g("q_target")))
        if mode == "double":
            actor.queue.append((g("next_tags"), g("q_online")))
        sets = getattr(target, "sets", 0)
        loss = alg.train()
        assert loss == float(g("loss")) and not actor.queue and not target.queue
        states, y_t = actor.trains[-1]
        assert np.array_equal(states[:, 0], g("tags"))                              # the sampled transitions
        ref = g("y_t")
        pick = np.argmax(g("q_online") if mode == "double" else g("q_target"), 1)
        maxq = g("q_target")[np.arange(len(pick)), pick]
        all_rewards = np.concatenate([golden["%s_msg%d_reward" % (mode, m)] for m in range(int(golden[mode + "_nmsg"]))])
        reward = all_rewards[g("tags").astype(int)]                                   # (a row's tag is its global index)
        bound = 4.0 * 2.0 ** -24 * (np.abs(reward) + np.abs(maxq))
        dy = np.abs(y_t.astype(np.float64) - ref.astype(np.float64))
        assert y_t.dtype == np.float32 and y_t.shape == ref.shape
        assert (dy <= bound[:, None]).all(), dy.max()
        assert (getattr(target, "sets", 0) > sets) == bool(g("target_updated"))       # the target-update cadence
        j += 1
    assert j == int(golden[mode + "_ntrain"]) and alg.train_count == int(golden[mode + "_train_count"])
    before = getattr(actor, "sets", 0), getattr(target, "sets", 0)
    alg.restore(model_weights={"phase": np.float64(42.0)})
    assert [getattr(actor, "sets", 0) - before[0], target.sets - before[1]] == list(golden["restore_sets"])
    assert [float(actor.weights["phase"]), float(target.weights["phase"])] == list(golden["restore_phase"])


def test_td_targets_is_the_numpy1_definition():
    from xingtian_amd.algorithm.dqn.dqn import td_targets
    rng = np.random.default_rng(0)
    r, q, d = rng.standard_normal(64), rng.standard_normal(64).astype(np.float32) * 5, rng.random(64) < 0.3
    want = np.array([np.float32(np.float64(r[i])) if d[i] else np.float32(np.float64(r[i]) + 0.99 * np.float64(q[i]))
                     for i in range(64)])
    got = td_targets(r, d, q, 0.99)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    assert np.array_equal(td_targets([1.0, 2.0], [2, 0], np.float32([3, 4]), 0.5), np.float32([1.0, 4.0]))   # truthiness


# ------------------------------------------------------------------------------------------------ CPU replica
@pytest.mark.parametrize("dueling", [False, True])
@pytest.mark.parametrize("a_dim", [2, 18])
def test_cpu_replica_predict_is_the_formula(dueling, a_dim):
    from xingtian_amd.model import model_builder
    info = {"model_name": "DqnMlp", "state_dim": [5], "action_dim": a_dim,
            "model_config": {"dueling": dueling, "DEVICE": "cpu", "SEED": 5, "HIDDEN_SIZE": 16, "NUM_LAYERS": 2}}
    model = model_builder(info)
    assert model.net.inference_only
    w = model.get_weights()
    rng = np.random.default_rng(a_dim)
    for k in w:
        if k.endswith("/bias"):
            w[k] = rng.standard_normal(w[k].shape).astype(np.float32) * 0.1
    model.set_weights(w)
    assert ("dense_3/kernel" in w) == dueling and w["dense_2/kernel"].shape == (16, a_dim)
    x = rng.standard_normal((7, 5)).astype(np.float32)
    h = x.astype(np.float64)
    for name in ("dense", "dense_1"):
        h = np.maximum(h @ w[name + "/kernel"] + w[name + "/bias"], 0.0)
    l = h @ w["dense_2/kernel"] + w["dense_2/bias"]
    q = l if not dueling else (h @ w["dense_3/kernel"] + w["dense_3/bias"]) + (l - l.mean(axis=1, keepdims=True))
    got = model.predict(x)
    assert got.dtype == np.float32 and got.shape == (7, a_dim)
    assert np.abs(got - q).max() <= 1e-5 * max(1.0, np.abs(q).max())
    with pytest.raises(RuntimeError):
        model.train_replay(None, None, None, 0.99, False)               # the replica has no update


# ------------------------------------------------------------------------------------------------ ABI
NEW_ENTRIES = ("xt_replay_gather", "xt_dqn_loss", "xt_net_dqn_step")
_CTYPE = {"int32_t": "c_int", "int64_t": "c_long", "double": "c_double", "float": "c_float"}


def test_abi_header_signatures_and_exported_symbols_agree_for_the_new_entries():
    import ctypes
    from xingtian_amd import lib as L
    with open(os.path.join(ROOT, "include", "xt_mi355x.h")) as f:
        header = f.read()
    assert re.search(r"#define XT_ABI_VERSION 12\b", header) and L.ABI_VERSION == 12
    handle = L.load()
    assert handle.xt_abi_version() == 12
    for name in NEW_ENTRIES:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        res, sig = L.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(sig) == len(args), (name, len(sig), len(args))
        for a, c in zip(args, sig):
            if "*" in a:                                  # every pointer is a void* or a typed struct pointer
                assert c is ctypes.c_void_p or hasattr(c, "contents"), (name, a, c)
                if "xt_dqn_cfg" in a:
                    assert c._type_ is L.DqnCfg
            else:
                ctype = _CTYPE[a.split()[0]]
                assert c.__name__ == ctype or (ctype == "c_long" and c is ctypes.c_int64) or \
                    (ctype == "c_int" and c is ctypes.c_int32), (name, a, c)
        assert getattr(handle, name) is not None           # exported
    # the struct mirrors the header field by field
    body = re.search(r"typedef struct xt_dqn_cfg \{(.*?)\} xt_dqn_cfg;", header, re.S).group(1)
    fields = [x.strip() for x in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if x.strip()]
    names = []
    for decl in fields:
        names += [n.strip(" *") for n in decl.split(None, 1)[1].split(",")]
    assert names == [n for n, _ in L.DqnCfg._fields_]
    assert ctypes.sizeof(L.DqnCfg) == 8 + 4 + 4 + 3 * 8


# ------------------------------------------------------------------------------------------------ the one reference head
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("dueling,double", [(False, False), (True, True)])
def test_dqn_loss_ref_without_weights_and_discounts_is_the_unit_weight_scalar_gamma_form_bit_for_bit(dtype, dueling, double):
    """``weights=None`` is a weight of one and ``disc=None`` is gamma in every row: a product with one is exact, so the
    weighted, per-sample-discount arithmetic of the single reference leaves the plain head's bits alone"""
    for seed in range(8):
        rng = np.random.default_rng(seed)
        b, a = int(rng.integers(1, 40)), int(rng.integers(1, 19))
        f = lambda *s: rng.standard_normal(s).astype(dtype)
        heads = [f(b, a), f(b), f(b, a) * 2, f(b), f(b, a) * 2 if double else None, f(b) if double else None]
        labels = (rng.integers(0, a, b), rng.standard_normal(b), rng.random(b) < 0.3, 0.99, dueling)
        plain = H.dqn_loss_ref(*heads, *labels)
        unit = H.dqn_loss_ref(*heads, *labels, np.ones(b), np.full(b, 0.99))
        for k, v in plain.items():
            assert np.asarray(v).dtype == np.asarray(unit[k]).dtype and np.asarray(v).tobytes() == np.asarray(unit[k]).tobytes(), k
        weighted = H.dqn_loss_ref(*heads, *labels, rng.uniform(0.05, 1.0, b))
        assert np.array_equal(weighted["delta"], plain["delta"]) and weighted["abs_td"] == plain["abs_td"]
