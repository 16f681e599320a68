"""CPU tests (no GPU) of the MuZero learner: the restated host functions against fixtures recorded by executing the
reference (tests/golden/muzero_host.npz, tools/gen_golden_muzero.py), the float64 checker's sensitivity to the four ways
of getting the unroll's gradient wrong, refusals, the registry, the example YAMLs' dicts, the C ABI and the CPU replica."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

from tests import muzero_helpers as MH
from tests.dqn_helpers import rel_max

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PONG = dict(value_range=(-21, 21), reward_range=(-2, 2))
DEFAULT = dict(value_range=(0, 60000), reward_range=(-300, 300))


@pytest.fixture(scope="module")
def golden(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "muzero_host.npz")))


# ---------------------------------------------------------------------- 1. host functions against the fixtures
def test_value_functions_match_the_reference(golden):
    from xingtian_amd.model.muzero import muzero_model as M
    assert np.array_equal(M.value_compression(golden["vc_x"]), golden["vc_y"])
    assert np.array_equal(M.value_decompression(golden["vc_x"]), golden["vd_y"])
    assert M.support_size(0, 60000) == 305 and M.support_size(-300, 300) == 26
    assert M.support_size(-21, 21) == 7 and M.support_size(-2, 2) == 3
    for i in range(4):
        support, vmin, vmax = golden["cv%d_cfg" % i]
        got = M.conver_value(golden["cv%d_in" % i], int(support), vmin, vmax)
        assert np.array_equal(got, golden["cv%d_out" % i]), i
        # the tests' own two-hot (the device's definition: each mass rounded to float32 once) is the same row
        assert np.abs(MH.two_hot(golden["cv%d_in" % i], int(support), vmin, vmax) - got).max() <= 6e-8
        support, vmin, vmax = golden["vt%d_cfg" % i]
        v = M.value_transform(golden["vt%d_in" % i], int(support), vmin, vmax)
        assert isinstance(v, float) and v == float(golden["vt%d_out" % i])


def test_conver_value_guards_the_top_of_the_range():
    """where the reference would index one past the row (the compressed value at or above the last bin), the whole mass
    goes on the last bin"""
    from xingtian_amd.model.muzero import muzero_model as M
    out = M.conver_value(np.array([[3.0, 0.0]]), 2, 0.0, 3.0)      # compress(3) = 1.003: floor 1 = support - 1
    assert np.array_equal(out, [[[0.0, 1.0], [1.0, 0.0]]])
    assert np.array_equal(MH.two_hot(np.array([[3.0, 0.0]]), 2, 0.0, 3.0), out)


class _Stub(object):
    td_step = 5

    def __init__(self):
        self.trains, self.fed = 0, None

    def value_inference(self, state):
        s = np.asarray(state, np.float64)
        return 0.01 * s.reshape(len(s), -1).sum(axis=1) + 0.5 * self.trains

    def train(self, state, label):
        self.fed = (state, label)
        self.trains += 1
        return 1.25


def _leaves(buf):
    return np.array([buf._sum[i] for i in range(buf._sum.capacity)], np.float64)


def test_seeded_algorithm_run_matches_the_reference(golden, monkeypatch):
    from xingtian_amd.algorithm.muzero import muzero as A
    import xingtian_amd.model as models
    stub = _Stub()
    monkeypatch.setattr(models, "model_builder", lambda info: stub)
    for k, v in (("BUFFER_SIZE", 8), ("BATCH_SIZE", 4), ("UNROLL_STEP", 5)):
        monkeypatch.setattr(A, k, v)
    alg = A.Muzero({"actor": {"state_dim": [4], "action_dim": 3}},
                   {"BUFFER_SIZE": 8, "BATCH_SIZE": 4, "UNROLL_STEP": 5, "instance_num": 1, "agent_num": 1})
    lens = [int(n) for n in golden["run_lens"]]
    keys = ("cur_state", "action", "reward", "root_value", "target_value", "child_visits")
    trajs = [{k: golden["run_traj_%d_%s" % (i, k)] for k in keys} for i in range(len(lens))]
    random.seed(11)
    for t in trajs:
        alg.prepare_data({k: (list(v) if k != "cur_state" else v) for k, v in t.items()})
    assert [lens.index(len(t["reward"])) for t in alg.buff._storage] == list(golden["run_stored"])      # the short one is dropped
    assert np.array_equal(_leaves(alg.buff), golden["run_outer_before"])
    mt = alg.make_target(int(golden["run_mt_index"]), alg.buff._storage[0])
    assert np.array_equal(np.array([m[0] for m in mt], np.float64), golden["run_mt_value"])
    assert np.array_equal(np.array([m[1] for m in mt], np.float64), golden["run_mt_reward"])
    assert np.array_equal(np.array([list(m[2]) if len(m[2]) else [0.0] * 3 for m in mt]), golden["run_mt_policy"])
    assert mt[-1] == (0, 0, [])                                     # absorbing past the end
    stored = list(alg.buff._storage)
    loss = alg.train()
    assert loss == float(golden["run_loss"])
    state, label = stub.fed
    assert np.array_equal(state[0], golden["run_image"]) and np.array_equal(state[1], golden["run_actions"])
    assert np.array_equal(state[2], golden["run_w"])
    assert np.array_equal(label[0], golden["run_values"]) and np.array_equal(label[1], golden["run_rewards"])
    assert np.array_equal(label[2], golden["run_policies"].astype(np.float32))
    assert np.array_equal(_leaves(alg.buff), golden["run_outer_after"])       # written at the batch positions 0 .. 3
    for k, t in enumerate(stored):
        assert np.array_equal(_leaves(t["pos_buff"]), golden["run_pos_after_%d" % k]), k


# ---------------------------------------------------------------------- 2. the checker is not blind
def test_checker_sees_each_wrong_variant():
    from xingtian_amd.model.muzero.muzero_model import mlp_spec
    spec = mlp_spec((4,), 2, 64, 4, 2, **PONG)
    w = MH.seeded_weights(spec, 3, bias_scale=0.3)
    obs, actions, tv, tr, tp = MH.make_batch(spec, 32, 4)
    twin = MH.Twin(spec, w)
    loss, ref = twin.loss_and_grads(obs.astype(np.float64), actions, tv, tr, tp)
    again = twin.loss_and_grads(obs.astype(np.float64), actions, tv, tr, tp)[1]
    assert all(np.array_equal(ref[k], again[k]) for k in ref)
    wrong = dict(hidden_scale_1=dict(hidden_scale=1.0), scale_on_h0=dict(scale_h0=True), no_step_factor=dict(step_factor=False),
                 reward_next_column=dict(reward_shift=1))
    for name, kw in wrong.items():
        bad = twin.loss_and_grads(obs.astype(np.float64), actions, tv, tr, tp, **kw)[1]
        worst = max(rel_max(bad[k], ref[k]) for k in ref if np.abs(ref[k]).max() > 0)
        print("{}: moves a gradient tensor by {:.3e}".format(name, worst))
        assert worst > 100 * MH.BAR_GRAD, name


# ---------------------------------------------------------------------- 3. refusals
def test_model_refusals():
    from xingtian_amd.model.muzero.muzero_model import cnn_spec, mlp_spec
    with pytest.raises(ValueError, match="td_step"):
        mlp_spec((4,), 2, 64, 4, 0, **PONG)
    with pytest.raises(ValueError, match="td_step"):
        mlp_spec((4,), 2, 64, 4, 17, **PONG)
    with pytest.raises(ValueError, match="action_dim"):
        mlp_spec((4,), 0, 64, 4, 5, **PONG)
    with pytest.raises(ValueError, match="max <= min"):
        mlp_spec((4,), 2, 64, 4, 5, value_range=(3, 3), reward_range=(-2, 2))
    with pytest.raises(ValueError, match="max <= min"):
        cnn_spec((84, 84, 4), 2, 256, 5, value_range=(0, 5), reward_range=(2, -2))
    with pytest.raises(ValueError, match=r"smallest valid one is \[36, 36, C\]"):
        cnn_spec((35, 36, 4), 2, 256, 5, **PONG)
    cnn_spec((36, 36, 4), 2, 256, 5, **PONG)
    with pytest.raises(ValueError, match="obs_type"):
        cnn_spec((84, 84, 4), 2, 256, 5, obs_type="int16", **PONG)


def _chain(L, layers):
    arr = (L.LayerDesc * len(layers))()
    for i, lay in enumerate(layers):
        for f in ("H", "W", "C", "KH", "KW", "S", "PT", "PL", "OH", "OW", "N"):
            setattr(arr[i].g, f, getattr(lay, f))
        arr[i].g.act = L.ACT[lay.act]
        arr[i].param_off = lay.param_off
    return arr


def _desc(L, spec, **over):
    chains = [_chain(L, c) for c in (spec.rep, spec.dyn, spec.pred)]
    d = L.MzDesc()
    d.n_rep, d.n_dyn, d.n_pred = len(spec.rep), len(spec.dyn), len(spec.pred)
    d.rep, d.dyn, d.pred = chains
    d.hidden, d.action_dim, d.unroll = spec.hidden, spec.action_dim, spec.unroll
    d.value_support, d.reward_support = spec.value_support, spec.reward_support
    d.obs_dim = spec.rep[0].H * spec.rep[0].W * spec.rep[0].C
    d.n_params = spec.n_flat
    d.value_min, d.value_max, d.reward_min, d.reward_max = spec.value_min, spec.value_max, spec.reward_min, spec.reward_max
    for k, v in over.items():
        setattr(d, k, v)
    return d, chains


def test_create_refusals_and_workspace():
    """xt_mz_create checks its description on the host: nothing is launched, no GPU is needed"""
    from xingtian_amd import lib as L
    from xingtian_amd.model.muzero.muzero_model import cnn_spec, mlp_spec
    lib = L.load()
    err = lambda: lib.xt_last_error().decode()      # noqa: E731
    spec = mlp_spec((4,), 2, 64, 4, 5, **PONG)

    def create(max_batch=8, **over):
        d, keep = _desc(L, spec, **over)
        h = ctypes.c_void_p()
        rc = lib.xt_mz_create(ctypes.byref(d), max_batch, ctypes.byref(h))
        return rc, h

    rc, h = create()
    assert rc == 0 and h.value
    assert lib.xt_mz_workspace_bytes(h) > 0 and lib.xt_mz_workspace_bytes(h) % 16 == 0
    p = ctypes.c_void_p(4096)
    assert lib.xt_mz_bind(h, p, p, p, p, p, p, 16) != 0 and "workspace" in err()
    assert lib.xt_mz_step(h, p, None, 4, p, p, p, p, ctypes.byref(L.MzCfg()), p, None) != 0 and "not bound" in err()
    lib.xt_mz_destroy(h)
    for over, word in ((dict(unroll=0), "unroll"), (dict(unroll=17), "unroll"), (dict(value_support=1), "support"),
                       (dict(reward_support=1), "support"), (dict(action_dim=0), "action_dim"),
                       (dict(value_max=-21.0), "max <= min"), (dict(reward_max=-2.0), "max <= min"), (dict(hidden=8), "hidden"),
                       (dict(n_dyn=2), "chain lengths"), (dict(n_params=spec.n_flat + 1), "n_params")):
        rc, h = create(**over)
        assert rc != 0 and word in err() and not h.value, (over, err())
    assert create(max_batch=0)[0] != 0 and "max_batch" in err()
    # the representation chain takes Dense layers only: a layer without output and a convolutional chain are refused
    d, keep = _desc(L, spec)
    keep[0][1].g.OH = 0
    h = ctypes.c_void_p()
    assert lib.xt_mz_create(ctypes.byref(d), 4, ctypes.byref(h)) != 0 and "not a Dense layer" in err()
    d, keep = _desc(L, cnn_spec((36, 36, 4), 2, 256, 5, **PONG))
    assert lib.xt_mz_create(ctypes.byref(d), 4, ctypes.byref(h)) != 0 and "rep layer 0 is not a Dense layer" in err()
    assert create(obs_dim=8)[0] != 0 and "rep layer 0 reads" in err()
    # the stand-alone entries refuse on the host as well
    assert lib.xt_mz_loss(p, 1, 4, 1, 1, p, None, 0.0, 1.0, 1.0, 1.0, None, p, p, None, None) != 0 and "N 1" in err()
    assert lib.xt_mz_cond_fwd(p, p, 1, 1, 4, 4, 0, 8, p, p, 1, p, None) != 0 and "xt_mz_cond_fwd" in err()
    assert lib.xt_mz_cond_bwd(p, p, 1, 2, 4, 4, 2, 8, p, p, p, 0.5, p, p, None, p, None) != 0 and "xt_mz_cond_bwd" in err()


def test_algorithm_refuses_another_unroll(monkeypatch):
    from xingtian_amd.algorithm.muzero import muzero as A
    import xingtian_amd.model as models
    monkeypatch.setattr(models, "model_builder", lambda info: _Stub())
    monkeypatch.setattr(A, "UNROLL_STEP", 5)
    cfg = {"instance_num": 1, "agent_num": 1}
    A.Muzero({"actor": {}}, dict(cfg))
    with pytest.raises(ValueError, match="UNROLL_STEP = 3 differs from the model's td_step = 5"):
        A.Muzero({"actor": {}}, dict(cfg, UNROLL_STEP=3))


# ---------------------------------------------------------------------- 4. registry, 5. YAML dicts
def test_registry_resolves_the_names():
    import xingtian_amd.algorithm  # noqa: F401
    import xingtian_amd.model  # noqa: F401
    from xingtian_amd.register import Registers
    assert Registers.algorithm["Muzero"].__name__ == "Muzero"
    assert Registers.model["MuzeroMlp"].__name__ == "MuzeroMlp" and Registers.model["MuzeroCnn"].__name__ == "MuzeroCnn"


YAML_MODELS = {
    "muzero_pong": dict(model_name="MuzeroCnn", state_dim=[84, 84, 4], action_dim=6, max_to_keep=500,
                        model_config=dict(reward_min=-2, reward_max=2, value_min=-21, value_max=21, obs_type="int8")),
    "muzero_breakout": dict(model_name="MuzeroCnn", state_dim=[84, 84, 4], action_dim=4, max_to_keep=500,
                            model_config=dict(reward_min=0, reward_max=50, value_min=0, value_max=500, obs_type="uint8")),
}


@pytest.mark.parametrize("name", sorted(YAML_MODELS))
def test_example_yaml_dicts_build_a_replica(name):
    from xingtian_amd.model import model_builder
    info = dict(YAML_MODELS[name])
    info["model_config"] = dict(info["model_config"], DEVICE="cpu", SEED=1)
    m = model_builder(info)
    assert m.net.inference_only and m.spec.unroll == 5 and m.spec.hidden == 256
    want = {"muzero_pong": (7, 3), "muzero_breakout": (m.spec.value_support, m.spec.reward_support)}[name]
    assert (m.spec.value_support, m.spec.reward_support) == want
    assert list(m.get_weights())[:8] == ["conv2d/kernel", "conv2d/bias", "conv2d_1/kernel", "conv2d_1/bias", "conv2d_2/kernel",
                                         "conv2d_2/bias", "dense/kernel", "dense/bias"]
    assert list(m.get_weights())[8:10] == ["dense_4/kernel", "dense_4/bias"]          # dynamics before prediction
    assert m.get_weights()["dense_4/kernel"].shape == (256 + info["action_dim"], 256)
    out = m.initial_inference(np.full((1, 84, 84, 4), 200, np.uint8))
    assert isinstance(out.value, float) and out.policy.shape == (info["action_dim"],) and out.hidden_state.shape == (256,)
    nxt = m.recurrent_inference(out.hidden_state, 1)
    assert isinstance(nxt.reward, float) and nxt.hidden_state.shape == (256,)
    with pytest.raises(RuntimeError, match="inference-only"):
        m.train([None, None, None], [None, None, None])


# ---------------------------------------------------------------------- 6. ABI
def test_abi_stays_12_and_the_table_matches_the_header():
    from xingtian_amd import lib as L
    header = open(os.path.join(ROOT, "include", "xt_mi355x.h")).read()
    assert re.search(r"#define XT_ABI_VERSION 12\b", header) and L.ABI_VERSION == 12
    section = header[header.index("MuZero: the unrolled model update"):]
    declared = set(re.findall(r"^(?:int|void|int64_t) (xt_mz_[a-z_]+)\(", section, re.M))
    in_table = {k for k in L.SIGNATURES if k.startswith("xt_mz_")}
    assert declared == in_table and len(declared) == 11
    assert list(L.SIGNATURES)[-2:] == ["xt_noisy_compose", "xt_noisy_grads"]          # the earlier pin still holds
    handle = L.load()
    ctype = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "float": ctypes.c_float}
    for name in sorted(declared):
        m = re.search(r"\b(int|void|int64_t) %s\(([^;]*)\);" % name, section)
        args = [a.strip() for a in m.group(2).replace("\n", " ").split(",")]
        res, sig = L.SIGNATURES[name]
        assert res is {"int": ctypes.c_int32, "void": None, "int64_t": ctypes.c_int64}[m.group(1)], name
        assert len(sig) == len(args), (name, len(sig), len(args))
        for a, c in zip(args, sig):
            if "*" in a:
                assert c is ctypes.c_void_p or (isinstance(c, type) and issubclass(c, ctypes._Pointer)), (name, a)
            else:
                assert c is ctype[a.split()[0]], (name, a)
        assert getattr(handle, name)
    assert int(re.search(r"#define XT_MZ_MAX_UNROLL (\d+)", header).group(1)) == L.MZ_MAX_UNROLL
    assert int(re.search(r"#define XT_MZ_WGRAD_ROWS (\d+)", header).group(1)) == L.MZ_WGRAD_ROWS == MH.WGRAD_ROWS
    fields = re.search(r"typedef struct xt_mz_desc \{(.*?)\} xt_mz_desc;", header, re.S).group(1)
    names = re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [n for n, _ in L.MzDesc._fields_]
    assert ctypes.sizeof(L.MzCfg) == 16


# ---------------------------------------------------------------------- 7. the CPU replica against float64
@pytest.mark.parametrize("kind", ["mlp", "cnn"])
def test_cpu_replica_matches_float64(kind):
    from xingtian_amd.model.muzero.muzero_model import CpuMuzero, cnn_spec, mlp_spec
    rng = np.random.default_rng(2)
    if kind == "mlp":
        spec, ot = mlp_spec((4,), 2, 64, 4, 5, **DEFAULT), "float32"
        obs = rng.standard_normal((6, 4)).astype(np.float32)
    else:
        spec, ot = cnn_spec((36, 36, 4), 6, 256, 5, obs_type="int8", **PONG), "int8"
        obs = rng.integers(0, 256, (6, 36, 36, 4)).astype(np.uint8)
    a, b = CpuMuzero(spec, seed=5), CpuMuzero(spec, seed=5)
    assert all(np.array_equal(v, b.get_weights()[k]) for k, v in a.get_weights().items())       # same seed, same weights
    w = MH.seeded_weights(spec, 6)
    a.set_weights(list(w.values()))                                                              # a list in the reference's order
    assert all(np.array_equal(v, w[k]) for k, v in a.get_weights().items())
    from xingtian_amd.model.muzero.muzero_model import obs_as_network_input
    twin = MH.Twin(spec, w)
    got = a.initial(obs_as_network_input(spec, obs, ot))
    ref = twin.initial(MH.network_input(spec, obs, ot))
    for g, r in zip(got, ref):
        assert rel_max(g, r) <= MH.BAR_LOSS
    acts = np.arange(6) % spec.action_dim
    for g, r in zip(a.recurrent(ref[2], acts), twin.recurrent(ref[2], acts)):
        assert rel_max(g, r) <= MH.BAR_LOSS
