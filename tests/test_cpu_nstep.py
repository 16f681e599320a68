"""n-step returns without a GPU: ``nstep_targets`` against the brute force of tests/nstep_helpers.py (exact), the
``follow`` ring of ``DeviceReplay``, the algorithm's host path with stub models, the configuration key and the C ABI of
the three new entries."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import nstep_helpers as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMA = N.GAMMA


@pytest.fixture(autouse=True)
def _module_constants_restored():
    """import_config overrides the modules' constants for the rest of the process: put them back"""
    from xingtian_amd.algorithm.dqn import dqn
    from xingtian_amd.model.dqn import dqn_cnn, dqn_mlp
    saved = [(m, {k: v for k, v in vars(m).items() if k.isupper()}) for m in (dqn, dqn_cnn, dqn_mlp)]
    yield
    for m, consts in saved:
        vars(m).update(consts)


# ------------------------------------------------------------------------------------------------ restatement
def test_the_case_table_holds_every_stop_cause_the_ring_end_and_the_oldest_row():
    c = N.cause_counts()
    print("n-step case table:", dict(c))
    for cause in N.CAUSES + ("wraps", "oldest"):
        assert c[cause] >= 1, cause
    for cap in (7, 50):
        lens = N.message_lengths(cap)
        assert {1, 2, 6} <= set(lens) and max(lens) > cap


@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("capacity", [7, 50])
def test_nstep_targets_equal_the_brute_force_exactly(capacity, n):
    from xingtian_amd.algorithm.dqn.dqn import DeviceReplay, nstep_targets
    ring, store = DeviceReplay(capacity, n_step=3), N.BruteStore(capacity)
    seen = set()
    for m in N.make_messages(capacity, 11):
        ring.add(m["cur_state"], m["next_state"], m["action"], m["reward"], m["done"])
        store.add(m)
        assert ring.size() == store.size() and ring.head == store.head()
        slots = store.live_slots()
        slots = slots[::-1] + slots[:3]                                     # unsorted, with duplicates
        got = nstep_targets(slots, *N.host_rings(ring), GAMMA, n, capacity)
        want, rows = store.targets(slots, n)
        assert [g.dtype for g in got] == [np.int32, np.int32, np.float64, np.float64, np.uint8]
        for g, w, name in zip(got, want, ("boot_slot", "action_n", "reward_n", "disc_n", "done_n")):
            assert np.array_equal(g, w), (name, g, w)                       # exactly
        seen |= {r["cause"] for r in rows}
        if n == 1:
            follow, action, reward, done = N.host_rings(ring)
            assert np.array_equal(got[0], slots) and np.array_equal(got[1], action[slots])
            assert np.array_equal(got[2], reward[slots]) and (got[3] == GAMMA).all() and np.array_equal(got[4], done[slots])
    if n > 1:
        assert seen >= set(N.CAUSES) - ({"done_mid"} if n == 2 else set())  # (n = 2 has no row between start and end)


def test_nstep_targets_treats_a_negative_follow_as_zero_and_a_slot_outside_the_ring_as_a_terminal_zero_row():
    from xingtian_amd.algorithm.dqn.dqn import nstep_targets
    follow, action = np.int32([2, -3, 0, 9]), np.int32([1, 2, 0, 1])
    reward, done = np.float64([1.0, 2.0, 4.0, 8.0]), np.uint8([0, 0, 0, 0])
    boot, act, rew, disc, dn = nstep_targets([1, 0, -1, 4, 3], follow, action, reward, done, 0.5, 3, 4)
    assert boot.tolist() == [1, 2, -1, 4, 1] and act.tolist() == [2, 1, 0, 0, 1]
    assert rew.tolist() == [2.0, 1.0 + 0.5 * 2.0 + 0.25 * 4.0, 0.0, 0.0, 8.0 + 0.5 * 1.0 + 0.25 * 2.0]      # 3 -> 0 -> 1: modulo
    assert disc.tolist() == [0.5, 0.125, 0.5, 0.5, 0.125] and dn.tolist() == [0, 0, 1, 1, 0]
    for n in (0, 257):
        with pytest.raises(ValueError):
            nstep_targets([0], follow, action, reward, done, 0.5, n, 4)


# ------------------------------------------------------------------------------------------------ DeviceReplay
@pytest.mark.parametrize("capacity", [7, 50])
def test_device_replay_keeps_follow_only_with_n_step_and_counts_its_bytes(capacity):
    from xingtian_amd.algorithm.dqn.dqn import DeviceReplay
    plain, ring = DeviceReplay(capacity), DeviceReplay(capacity, n_step=3)
    assert plain.n_step == 1 and ring.n_step == 3 and plain.follow is None and ring.follow is None       # allocated at the first add
    store = N.BruteStore(capacity)
    for m in N.make_messages(capacity, 11):
        for r in (plain, ring):
            r.add(m["cur_state"], m["next_state"], m["action"], m["reward"], m["done"])
        store.add(m)
        live = store.live_slots()
        assert ring.follow.dtype.is_floating_point is False and ring.follow.shape == (capacity,)
        assert ring.follow[live].tolist() == [store.follow()[s] for s in live]                              # wrapped and evicted writes
        assert (plain.head, plain.size()) == (ring.head, ring.size())
        random.seed(capacity + store.written)
        a = plain.sample(min(plain.size(), 5))
        random.seed(capacity + store.written)
        assert ring.sample(min(ring.size(), 5)) == a                        # the same draw
    assert store.evicted and plain.follow is None
    row_bytes = 2 * 4
    assert plain.bytes == capacity * (2 * row_bytes + 13) and ring.bytes == plain.bytes + 4 * capacity
    for name in ("cur_state", "next_state", "action", "reward", "done"):
        assert np.array_equal(getattr(plain, name).numpy(), getattr(ring, name).numpy())


# ------------------------------------------------------------------------------------------------ host path
def _q(tags, role, a_dim=3):
    """the stub models' Q values: a fixed function of the row's tag, the action and the network"""
    t = np.asarray(tags, np.float64).reshape(-1, 1)
    return np.sin(t * 0.37 + np.arange(a_dim) * 1.3 + (0.0 if role == "actor" else 2.1)).astype(np.float32) * 3.0


class _TagModel(object):
    """reference-style model (``predict`` / ``train(states, y_t)`` only): records what it is asked"""
    instances = []

    def __init__(self, model_info):
        self.role = "actor" if not _TagModel.instances else "target"
        _TagModel.instances.append(self)
        self.asked, self.trains = [], []

    def predict(self, state):
        tags = np.asarray(state)[:, 0].astype(np.float64)
        self.asked.append(tags)
        return _q(tags, self.role)

    def train(self, state, label):
        self.trains.append((np.array(state), np.array(label)))
        return 0.25

    def get_weights(self):
        return {}

    def set_weights(self, w):
        pass


def _host_alg(**cfg):
    from xingtian_amd.algorithm import alg_builder
    from xingtian_amd.register import Registers
    _TagModel.instances = []
    Registers.model._by_name["_TagModel"] = _TagModel
    try:
        base = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1, "BUFFER_SIZE": 50, "BATCH_SIZE": 16,
                "GAMMA": GAMMA, "TARGET_UPDATE_FREQ": 100}
        base.update(cfg)
        return alg_builder("DQN", {"actor": {"model_name": "_TagModel", "state_dim": [2], "action_dim": 3}}, base)
    finally:
        del Registers.model._by_name["_TagModel"]


@pytest.mark.parametrize("double", [False, True])
def test_host_path_hands_the_brute_force_targets_to_train_and_the_boot_rows_to_predict(double):
    alg = _host_alg(n_step=3, double_dqn=double)
    assert not alg.device_step and alg.n_step == 3 and alg.buff.n_step == 3
    store = N.BruteStore(50)
    for m in N.make_messages(50, 11):
        alg.prepare_data(m)
        store.add(m)
    causes = set()
    for t in range(3):
        random.seed(40 + t)
        slots = alg.buff.sample(16)
        random.seed(40 + t)
        assert alg.train() == 0.25
        rows = [store.target(s, 3) for s in slots]
        causes |= {r["cause"] for r in rows}
        tags, next_tags = np.float64([r["tag"] for r in rows]), np.float64([r["next_tag"] for r in rows])
        actor, target = alg.actor, alg.target_actor
        assert np.array_equal(actor.asked.pop(0), tags)                     # the states of the start rows
        assert np.array_equal(target.asked.pop(0), next_tags)               # the next states of the boot rows
        if double:
            assert np.array_equal(actor.asked.pop(0), next_tags)
        assert not actor.asked and not target.asked
        q_t = _q(next_tags, "target")
        pick = np.argmax(_q(next_tags, "actor") if double else q_t, 1)
        want = _q(tags, "actor")
        for i, r in enumerate(rows):
            boot = r["reward"] + r["disc"] * float(q_t[i, pick[i]])         # float64, then one rounding
            want[i, r["action"]] = np.float32(r["reward"] if r["done"] else boot)
        states, y_t = actor.trains[-1]
        assert np.array_equal(states[:, 0], tags) and y_t.dtype == np.float32
        assert np.array_equal(y_t, want)                                    # exactly
    assert causes >= {"full", "done_start", "message_end"} and alg.train_count == 3


def test_td_targets_takes_a_per_sample_discount_and_keeps_the_scalar_result():
    from xingtian_amd.algorithm.dqn.dqn import td_targets
    rng = np.random.default_rng(1)
    r, q, d = rng.standard_normal(32), rng.standard_normal(32).astype(np.float32) * 5, rng.random(32) < 0.3
    scalar = td_targets(r, d, q, 0.99)
    want = np.array([np.float32(r[i]) if d[i] else np.float32(r[i] + 0.99 * np.float64(q[i])) for i in range(32)])
    assert np.array_equal(scalar, want) and np.array_equal(td_targets(r, d, q, np.full(32, 0.99)), scalar)
    g = 0.99 ** rng.integers(1, 4, 32)
    want = np.array([np.float32(r[i]) if d[i] else np.float32(r[i] + g[i] * np.float64(q[i])) for i in range(32)])
    assert np.array_equal(td_targets(r, d, q, g), want)


# ------------------------------------------------------------------------------------------------ configuration
def test_n_step_defaults_to_one_and_bad_values_raise_value_error_naming_them():
    alg = _host_alg()
    assert alg.n_step == 1 and alg.buff.n_step == 1 and alg.buff.follow is None
    assert _host_alg(n_step=256).n_step == 256 and _host_alg(n_step=1).buff.follow is None
    for bad in (0, 257, 2.5):
        with pytest.raises(ValueError) as info:
            _host_alg(n_step=bad)
        assert "n_step" in str(info.value) and repr(bad) in str(info.value)
    from xingtian_amd.algorithm.dqn import default_config
    assert not hasattr(default_config, "N_STEP")


def test_a_host_train_without_n_step_is_the_one_step_train():
    alg = _host_alg()
    msgs = N.make_messages(50, 11)
    for m in msgs:
        alg.prepare_data(m)
    random.seed(3)
    slots = alg.buff.sample(16)
    random.seed(3)
    alg.train()
    assert np.array_equal(alg.target_actor.asked[0], alg.buff.next_state[slots][:, 0].numpy().astype(np.float64))


# ------------------------------------------------------------------------------------------------ ABI
NEW_ENTRIES = ("xt_replay_gather_nstep", "xt_dqn_loss_n", "xt_net_dqn_step_n")
_CTYPE = {"int32_t": "c_int", "int64_t": "c_long", "double": "c_double", "float": "c_float"}


def test_abi_header_signatures_and_exported_symbols_agree_for_the_nstep_entries():
    from xingtian_amd import lib as L
    with open(os.path.join(ROOT, "include", "xt_mi355x.h")) as f:
        header = f.read()
    assert re.search(r"#define XT_ABI_VERSION 12\b", header) and L.ABI_VERSION == 12
    handle = L.load()
    assert handle.xt_abi_version() == 12
    structs = {"xt_dqn_cfg": L.DqnCfg, "xt_per_cfg": L.PerCfg, "xt_nstep_cfg": L.NstepCfg}
    for name in NEW_ENTRIES:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, header)
        assert m, name
        args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
        res, sig = L.SIGNATURES[name]
        assert res is ctypes.c_int32 and len(sig) == len(args), (name, len(sig), len(args))
        for a, c in zip(args, sig):
            if "*" in a:                                  # every pointer is a void* or a typed struct pointer
                assert c is ctypes.c_void_p or hasattr(c, "contents"), (name, a, c)
                for sname, stype in structs.items():
                    if sname in a:
                        assert c._type_ is stype, (name, a)
            else:
                ctype = _CTYPE[a.split()[0]]
                assert c.__name__ == ctype or (ctype == "c_long" and c is ctypes.c_int64) or \
                    (ctype == "c_int" and c is ctypes.c_int32), (name, a, c)
        assert getattr(handle, name) is not None           # exported
    body = re.search(r"typedef struct xt_nstep_cfg \{(.*?)\} xt_nstep_cfg;", header, re.S).group(1)
    fields = [x.strip() for x in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if x.strip()]
    names = [d.replace("const ", "").split(None, 1)[1].strip(" *") for d in fields]
    assert names == [n for n, _ in L.NstepCfg._fields_] == ["n", "follow", "boot_slots", "action_n", "reward_n", "disc_n",
                                                            "done_n"]
    for (n, ct), d in zip(L.NstepCfg._fields_, fields):
        assert (ct is ctypes.c_void_p) == ("*" in d), n
    assert ctypes.sizeof(L.NstepCfg) == 8 + 6 * 8
    # the earlier entries keep their shapes; the new head is the weighted one plus one pointer
    assert len(L.SIGNATURES["xt_dqn_loss_w"][1]) == 23 and len(L.SIGNATURES["xt_dqn_loss_n"][1]) == 24
    assert len(L.SIGNATURES["xt_net_dqn_step"][1]) == 15 and len(L.SIGNATURES["xt_net_dqn_step_per"][1]) == 16
    assert ctypes.sizeof(L.DqnCfg) == 40 and ctypes.sizeof(L.PerCfg) == 88
