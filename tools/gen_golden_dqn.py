"""Golden vectors of the reference's DQN host logic, produced by EXECUTING the reference.

``xt/algorithm/dqn/dqn.py::DQN`` and ``xt/algorithm/replay_buffer.py::ReplayBuffer`` (with the real ``Algorithm`` base
class, ``import_config`` and ``xt/algorithm/dqn/default_config.py``) are loaded with importlib under the stubs of
``oracle/gen_golden_alg.py``.  ``xt.model.model_builder`` returns a recording model whose ``predict`` returns
deterministic float32 Q values (a function of the row's tag -- element 0 of the state -- and of the model's "weights",
one phase number that ``set_weights`` copies, so a target update is visible) and whose ``train`` stores what it is
handed.  The script runs ``prepare_data`` / ``train`` sequences with a small BUFFER_SIZE that wraps around (one message
is longer than the buffer) for both ``double_dqn`` settings and writes tests/golden/alg_dqn.npz:

    seed                                            random.seed before the sequence
    <mode>_nmsg, <mode>_msg<i>_<field>              the messages, in order
    <mode>_script                                   the sequence: entry >= 0 = prepare_data(message i), -1 = train
    <mode>_train<j>_tags / _next_tags               tag of every sampled state / next state, in sample order
    <mode>_train<j>_y_pred / _q_target / _q_online  what the three predicts returned (q_online: double_dqn only)
    <mode>_train<j>_y_t / _loss / _target_updated   the label handed to Model.train, the returned loss, whether the target
                                                    network received weights in this train
    restore_*                                       restore(model_weights=...) reaches both networks

and tests/golden/dqn_configs.json: the parsed DQN example YAMLs and the values of the two ``default_config`` modules.
Nothing at test time reads the reference tree.

Usage:  python tools/gen_golden_dqn.py
"""
import json
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden_alg as ga  # noqa: E402

A_DIM, SEED = 3, 20240607
ALG_CFG = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1, "BUFFER_SIZE": 8, "BATCH_SIZE": 4,
           "TARGET_UPDATE_FREQ": 2}
MODEL_INFO = {"actor": {"model_name": "RecordingDqnModel", "state_dim": [3], "action_dim": A_DIM}}
MESSAGES = (5, 6, 10, 3)                       # rows per message: below, across and beyond a buffer of 8
SCRIPT = (0, -1, 1, -1, -1, 2, -1, 3, -1, -1)   # message index, or -1 = train
YAMLS = ["examples/beamrider_dqn.yaml", "examples/breakout_dqn.yaml", "examples/cartpole_dqn.yaml",
         "examples/pong_dqn.yaml", "examples/qbert_dqn.yaml", "examples/spaceinvader_dqn.yaml",
         "examples/evolution/pbt_spaceinvader_dqn.yaml", "examples/evolution/pbt_spaceinvader_dqn_25.yaml"]


class RecordingDqnModel(object):
    built = 0

    def __init__(self, model_info):
        self.a_dim = model_info["action_dim"]
        self.phase = float(RecordingDqnModel.built)          # actor 0.0, target 1.0
        RecordingDqnModel.built += 1
        self.predicts, self.trains, self.sets = [], [], 0

    def predict(self, state):
        tags = np.asarray(state)[:, 0].astype(np.float64)
        q = np.sin(tags[:, None] * 0.37 * (np.arange(self.a_dim) + 1.0) + self.phase) * 3.0
        q = q.astype(np.float32)
        self.predicts.append((np.array(state, copy=True), q.copy()))
        return q

    def train(self, state, label):
        self.trains.append((np.array(state, copy=True), np.array(label, copy=True)))
        self.phase += 0.25                                   # "learning": the next predictions differ
        return 0.5 + len(self.trains)

    def get_weights(self):
        return {"phase": np.float64(self.phase)}

    def set_weights(self, weights):
        self.phase = float(weights["phase"])
        self.sets += 1


def load_reference_dqn():
    ga.load_reference_algorithms()             # the stubs and the real Algorithm base class / import_config
    sys.modules["xt.model"].model_builder = lambda model_info: RecordingDqnModel(model_info)
    base = sys.modules["xt.algorithm.algorithm"]           # (the base class bound the factory when it was imported)
    if hasattr(base, "model_builder"):
        base.model_builder = sys.modules["xt.model"].model_builder
    pkg = type(sys)("xt.algorithm.dqn")
    pkg.__path__ = []
    sys.modules["xt.algorithm.dqn"] = pkg
    ga._load("xt.algorithm.dqn.default_config", "xt/algorithm/dqn/default_config.py")
    ga._load("xt.algorithm.replay_buffer", "xt/algorithm/replay_buffer.py")
    return ga._load("xt.algorithm.dqn.dqn", "xt/algorithm/dqn/dqn.py").DQN


def messages(seed=7):
    rng = np.random.default_rng(seed)
    out, tag = [], 0
    for n in MESSAGES:
        tags = np.arange(tag, tag + n, dtype=np.float32)
        tag += n
        cur = np.stack([tags, rng.standard_normal(n).astype(np.float32), np.zeros(n, np.float32)], axis=1)
        nxt = cur.copy()
        nxt[:, 0] += 1000.0                                  # the next state's tag
        out.append({"cur_state": cur, "next_state": nxt, "action": rng.integers(0, A_DIM, n).astype(np.int32),
                    "reward": [float(x) for x in rng.choice([-1.0, 0.0, 0.1, 0.7, 1.0], n)],
                    "done": [bool(x) for x in (rng.random(n) < 0.3)]})
    return out


def run(DQN, double, out):
    mode = "double" if double else "plain"
    RecordingDqnModel.built = 0
    cfg = dict(ALG_CFG)
    if double:
        cfg["double_dqn"] = True
    alg = DQN(dict(MODEL_INFO), cfg)
    msgs = messages()
    out[mode + "_nmsg"] = np.int64(len(msgs))
    for i, m in enumerate(msgs):
        for k, v in m.items():
            out["%s_msg%d_%s" % (mode, i, k)] = np.asarray(v)
    out[mode + "_script"] = np.asarray(SCRIPT, np.int64)
    random.seed(SEED)
    j = 0
    for step in SCRIPT:
        if step >= 0:
            alg.prepare_data(msgs[step])
            continue
        actor, target = alg.actor, alg.target_actor
        np_a, np_t, sets = len(actor.predicts), len(target.predicts), target.sets
        loss = alg.train()
        pre = "%s_train%d_" % (mode, j)
        states, y_t = actor.trains[-1]
        out[pre + "tags"], out[pre + "y_t"], out[pre + "loss"] = states[:, 0].copy(), y_t, np.float64(loss)
        out[pre + "y_pred"] = actor.predicts[np_a][1]
        out[pre + "next_tags"] = target.predicts[np_t][0][:, 0].copy()
        out[pre + "q_target"] = target.predicts[np_t][1]
        if double:
            out[pre + "q_online"] = actor.predicts[np_a + 1][1]
        out[pre + "target_updated"] = np.bool_(target.sets > sets)
        out[pre + "size"] = np.int64(alg.buff.size())
        j += 1
    out[mode + "_ntrain"] = np.int64(j)
    out[mode + "_train_count"] = np.int64(alg.train_count)
    return alg


def defaults_of(path):
    ns = {}
    with open(os.path.join(ga.REF, path)) as f:
        exec(compile(f.read(), path, "exec"), ns)
    return {k: v for k, v in ns.items() if k.isupper()}


def main():
    import yaml
    DQN = load_reference_dqn()
    out = {"seed": np.int64(SEED), "gamma": np.float64(sys.modules["xt.algorithm.dqn.dqn"].GAMMA)}
    for k, v in ALG_CFG.items():
        out["cfg_" + k] = np.int64(v)
    run(DQN, False, out)
    alg = run(DQN, True, out)
    before = alg.actor.sets, alg.target_actor.sets
    alg.restore(model_weights={"phase": np.float64(42.0)})
    out["restore_sets"] = np.asarray([alg.actor.sets - before[0], alg.target_actor.sets - before[1]], np.int64)
    out["restore_phase"] = np.asarray([alg.actor.phase, alg.target_actor.phase], np.float64)
    np.savez_compressed(os.path.join(ga.OUT, "alg_dqn.npz"), **out)
    configs = {}
    for y in YAMLS:
        with open(os.path.join(ga.REF, y)) as f:
            configs[y] = yaml.safe_load(f)
    with open(os.path.join(ga.OUT, "dqn_configs.json"), "w") as f:
        json.dump({"yamls": configs, "defaults": {"algorithm/dqn": defaults_of("xt/algorithm/dqn/default_config.py"),
                                                  "model/dqn": defaults_of("xt/model/dqn/default_config.py")}},
                  f, indent=1, sort_keys=True)
    print("wrote alg_dqn.npz (%d + %d trains) and dqn_configs.json" % (int(out["plain_ntrain"]), int(out["double_ntrain"])))


if __name__ == "__main__":
    main()
