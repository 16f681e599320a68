"""Golden vectors of the reference's MuZero HOST code, produced by EXECUTING the reference.

Loaded by path under stub packages (the pattern of ``tools/gen_golden_per.py``): ``xt/model/muzero/muzero_utils.py``,
``xt/model/muzero/muzero_model.py`` (for ``conver_value`` / ``value_transform``; its TensorFlow / Keras imports are empty
stubs, nothing of the graph is built), ``xt/algorithm/muzero/muzero.py`` with ``default_config.py``,
``xt/algorithm/prioritized_replay_buffer_muzero.py`` and ``xt/algorithm/segment_tree.py``.  ``xt.algorithm.Algorithm`` is
a stub that takes the model it is given.  ``np.asscalar`` (gone from NumPy) is supplied as ``ndarray.item``.

Recorded in tests/golden/muzero_host.npz (data only; nothing at test time reads the reference):
  vc_x, vc_y, vd_y        value_compression / value_decompression of vc_x
  cv<i>_in / _cfg / _out  conver_value of scalars [B, T] with (support, min, max); no entry touches the top bin's neighbour
  vt<i>_in / _cfg / _out  value_transform of a support row
  The seeded run (BUFFER_SIZE 8, BATCH_SIZE 4, UNROLL_STEP 5, random.seed(11)) against the stub model below:
  run_lens                lengths of the 6 trajectories handed to prepare_data (one is too short and is dropped)
  run_traj_<k>_*          the trajectories' arrays (cur_state, action, reward, root_value, target_value, child_visits)
  run_outer_before        the outer buffer's sum-tree leaves before the train
  run_mt_index / run_mt_* make_target of trajectory 0 at a position near its end (absorbing states: policy rows empty -> zeros)
  run_stored              which of the handed trajectories every slot of the outer buffer holds
  run_w                   the importance weights handed to the model; run_image / run_actions / run_values / run_rewards /
                          run_policies the arrays of the train (they pin the sampled trajectories and positions)
  run_outer_after         the outer leaves after update_pri (written at the batch POSITIONS 0 .. 3)
  run_pos_after_<k>       the leaves of every stored trajectory's pos_buff after update_pri
  run_loss                what train returned (the stub's constant)

The stub model: value_inference(state) = 0.01 * sum(state) + 0.5 * (number of trains so far); train returns 1.25.

Usage:  python tools/gen_golden_muzero.py [reference root]
"""
import importlib.util
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 11


class StubModel(object):
    def __init__(self):
        self.trains = 0
        self.fed = None

    def value_inference(self, state):
        s = np.asarray(state, np.float64)
        return 0.01 * s.reshape(len(s), -1).sum(axis=1) + 0.5 * self.trains

    def train(self, state, label):
        self.fed = (state, label)
        self.trains += 1
        return 1.25


def _package(name):
    if name not in sys.modules:
        pkg = type(sys)(name)
        pkg.__path__ = []
        sys.modules[name] = pkg
    return sys.modules[name]


def _load(ref, name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, path))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref):
    for name in ("xt", "xt.model", "xt.model.muzero", "xt.algorithm", "xt.algorithm.muzero", "zeus", "zeus.common",
                 "zeus.common.util"):
        _package(name)
    if not hasattr(np, "asscalar"):
        np.asscalar = lambda a: a.item()

    class _Anything(object):
        def __init__(self, *a, **k):
            pass

        def __getattr__(self, name):
            return _Anything()

        def __call__(self, *a, **k):
            return _Anything()

    compat = _package("xt.model.tf_compat")
    for n in ("tf", "K", "MSE"):
        setattr(compat, n, _Anything())
    for n in ("Dense", "Model", "Sequential", "Input", "Lambda", "Conv2D", "Flatten"):
        setattr(compat, n, type(n, (object,), {}))
    base = _package("xt.model.model")
    base.XTModel = type("XTModel", (object,), {})
    base.check_keep_model = lambda *a, **k: None
    common = _package("zeus.common.util.common")

    def import_config(global_para, config):
        for k, v in (config or {}).items():
            if k in global_para:
                global_para[k] = v
    common.import_config = import_config
    reg = _package("zeus.common.util.register")

    class _Reg(object):
        model = staticmethod(lambda c: c)
        algorithm = staticmethod(lambda c: c)
    reg.Registers = _Reg
    _load(ref, "xt.model.muzero.default_config", "xt/model/muzero/default_config.py")
    utils = _load(ref, "xt.model.muzero.muzero_utils", "xt/model/muzero/muzero_utils.py")
    model = _load(ref, "xt.model.muzero.muzero_model", "xt/model/muzero/muzero_model.py")

    class Algorithm(object):
        def __init__(self, alg_name, model_info, alg_config, **kw):
            self.actor = model_info["stub"]
    sys.modules["xt.algorithm"].Algorithm = Algorithm
    rb = _package("xt.algorithm.replay_buffer")
    rb.ReplayBuffer = type("ReplayBuffer", (object,), {})
    _load(ref, "xt.algorithm.segment_tree", "xt/algorithm/segment_tree.py")
    _load(ref, "xt.algorithm.prioritized_replay_buffer_muzero", "xt/algorithm/prioritized_replay_buffer_muzero.py")
    _load(ref, "xt.algorithm.muzero.default_config", "xt/algorithm/muzero/default_config.py")
    alg = _load(ref, "xt.algorithm.muzero.muzero", "xt/algorithm/muzero/muzero.py")
    return utils, model.MuzeroModel, alg.Muzero


def trajectory(rng, length, a=3):
    visits = rng.random((length, a))
    return dict(cur_state=rng.uniform(-1, 1, (length, 4)), action=rng.integers(0, a, length),
                reward=rng.uniform(-2, 2, length), root_value=rng.uniform(-21, 21, length),
                target_value=rng.uniform(-21, 21, length), child_visits=visits / visits.sum(axis=1, keepdims=True))


def leaves(buf):
    cap = buf._it_sum._capacity
    return np.array([buf._it_sum[i] for i in range(cap)], np.float64)


def main(ref):
    utils, Model, Muzero = load_reference(ref)
    out = {}
    x = np.concatenate([np.linspace(-50, 700, 61), [0.0, 1e-9, 3.0, 42.0, 600.0, 60000.0]])
    out["vc_x"], out["vc_y"], out["vd_y"] = x, utils.value_compression(x), utils.value_decompression(x)
    rng = np.random.default_rng(SEED)
    for i, (vmin, vmax) in enumerate([(-21, 21), (0, 60000), (-300, 300), (-2, 2)]):
        support = int(np.ceil(utils.value_compression(vmax - vmin))) + 1
        t = rng.uniform(vmin - 3, vmax - 1e-3 * (vmax - vmin), (5, 6))
        t[0, 0], t[0, 1] = vmin, vmin - 10.0
        out["cv%d_in" % i], out["cv%d_cfg" % i] = t, np.array([support, vmin, vmax], np.float64)
        out["cv%d_out" % i] = Model.conver_value(None, t, support, vmin, vmax)
        row = rng.random(support)
        row /= row.sum()
        out["vt%d_in" % i], out["vt%d_cfg" % i] = row, np.array([support, vmin, vmax], np.float64)
        out["vt%d_out" % i] = np.float64(Model.value_transform(None, row, support, vmin, vmax))
    # ---- the seeded run
    stub = StubModel()
    alg = Muzero({"actor": {"stub": stub}}, {"BUFFER_SIZE": 8, "BATCH_SIZE": 4, "UNROLL_STEP": 5})
    lens = [12, 9, 6, 15, 8, 20]
    out["run_lens"] = np.array(lens)
    trajs = [trajectory(rng, n) for n in lens]
    for k, t in enumerate(trajs):
        for key, v in t.items():
            out["run_traj_%d_%s" % (k, key)] = np.asarray(v)
    random.seed(SEED)
    for t in trajs:
        alg.prepare_data({k: (list(v) if k != "cur_state" else v) for k, v in t.items()})
    stored = list(alg.buff._storage)
    out["run_stored"] = np.array([lens.index(len(t["reward"])) for t in stored])
    out["run_outer_before"] = leaves(alg.buff)
    mt = alg.make_target(9, stored[0])
    out["run_mt_index"] = np.array(9)
    out["run_mt_value"] = np.array([m[0] for m in mt], np.float64)
    out["run_mt_reward"] = np.array([m[1] for m in mt], np.float64)
    out["run_mt_policy"] = np.array([list(m[2]) if len(m[2]) else [0.0] * 3 for m in mt], np.float64)
    # record what sample() and sample_position() drew by wrapping the model's train
    loss = alg.train()
    state, label = stub.fed
    out["run_loss"] = np.float64(loss)
    out["run_image"], out["run_actions"], out["run_w"] = np.asarray(state[0]), np.asarray(state[1]), np.asarray(state[2])
    out["run_values"], out["run_rewards"] = np.asarray(label[0], np.float64), np.asarray(label[1], np.float64)
    out["run_policies"] = np.asarray(label[2], np.float64)
    out["run_outer_after"] = leaves(alg.buff)
    for k, t in enumerate(stored):
        out["run_pos_after_%d" % k] = leaves(t["pos_buff"])
    os.makedirs(GOLDEN, exist_ok=True)
    path = os.path.join(GOLDEN, "muzero_host.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("XT_REFERENCE", "reference"))
