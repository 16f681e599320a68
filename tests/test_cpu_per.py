"""Prioritised replay without a GPU: the restatement of tests/per_helpers.py against what the executed reference
recorded (tests/golden/per_cases.npz), the C ABI of the new entries, and the algorithm's configuration and refusals."""
import os
import re

import numpy as np
import pytest

import per_helpers as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("c5", "c37", "c707", "c1000", "c64", "c37_alpha1", "c37_beta1", "c64_edge")


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
def cases(golden_dir):
    return P.load_cases(golden_dir)


# ------------------------------------------------------------------------------------------------ restatement
def test_the_golden_file_holds_the_cases_of_the_issue(cases):
    assert sorted(cases) == sorted(NAMES)
    shape = lambda c: (c.capacity, c.n, c.b, c.alpha, c.beta)
    assert shape(cases["c5"]) == (5, 5, 32, 0.6, 0.4) and shape(cases["c37"]) == (37, 37, 33, 0.6, 0.4)
    assert shape(cases["c707"]) == (1000, 707, 256, 0.6, 0.4) and shape(cases["c1000"]) == (1000, 1000, 1, 0.6, 0.4)
    assert shape(cases["c64"]) == (64, 64, 32, 0.6, 0.4) and shape(cases["c64_edge"]) == (64, 64, 32, 0.6, 0.4)
    assert cases["c37_alpha1"].alpha == 1.0 and cases["c37_beta1"].beta == 1.0
    assert max(cases["c5"].msg_lens) > 5                                   # one message longer than the capacity
    edge = cases["c64_edge"].u
    assert edge[0] == 0.0 and edge[-1] == 1.0 - 2.0 ** -53 and edge[1] == 1.0 - 2.0 ** -53 and edge[2] == 0.0
    for c in cases.values():
        assert sum(c.msg_lens) > c.capacity or c.n < c.capacity            # the adds wrap the ring, or it is not full
        assert sum(len(b[0]) for b in c.batches) >= 3 * c.n and max(c.idx) < c.n
        assert all(len(set(b[0])) < len(b[0]) for b in c.batches if len(b[0]) > c.n)      # duplicates within a batch


@pytest.mark.parametrize("name", NAMES)
def test_restatement_on_the_recorded_leaves_is_the_reference_bit_for_bit(cases, name):
    c = cases[name]
    s, m = P.build_trees(c.leaves.tolist())
    assert s == c.sum.tolist() and m == c.min.tolist()                     # both full trees
    p_total, slots, weights = P.sample(s, m, c.n, c.u, c.beta)
    assert p_total == c.p_total and slots == c.idx
    assert P.rel_err(weights, c.w) <= 1e-12
    assert P.prefix_total(s, c.n) == P.prefix_total(c.sum.tolist(), c.n)


@pytest.mark.parametrize("name", NAMES)
def test_leaves_from_the_recorded_priorities(cases, name):
    c = cases[name]
    leaves, max_prio = c.host_leaves()
    assert max_prio == c.max_prio                                          # exact: a maximum of recorded values
    written = c.leaves != 0.0
    assert written.sum() == c.n and not np.asarray(leaves)[~written].any()
    assert P.rel_err(np.asarray(leaves)[written], c.leaves[written]) <= 1e-12


def test_the_last_stored_slot_is_outside_the_mass_range(cases):
    c = cases["c5"]
    s, _ = P.build_trees(c.leaves.tolist())
    assert P.prefix_total(s, c.n) == s[2] == c.p_total                     # leaves [0, 3] of 5 stored: one subtree
    assert set(c.idx) == {0, 1, 2, 3}                                      # slot 4 is stored and never drawn
    big = cases["c707"]
    s, _ = P.build_trees(big.leaves.tolist())
    # leaves [0, 705]: 512 + 128 + 64 + 2 -> nodes 2, 12 (of 1024: [512, 640)), 26, and the pair's parent
    parts = [s[2], s[(1024 + 512) >> 7], s[(1024 + 640) >> 6], s[(1024 + 704) >> 1]]
    want = parts[0] + (parts[1] + (parts[2] + parts[3]))
    assert P.prefix_total(s, big.n) == want == big.p_total


# ------------------------------------------------------------------------------------------------ ABI
NEW_ENTRIES = ("xt_per_add", "xt_per_sample", "xt_per_update", "xt_dqn_loss_w", "xt_net_dqn_step_per")
_CTYPE = {"int32_t": "c_int", "int64_t": "c_long", "double": "c_double", "float": "c_float"}


def test_abi_header_signatures_and_exported_symbols_agree_for_the_per_entries():
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
                if "xt_per_cfg" in a:
                    assert c._type_ is L.PerCfg
            else:
                ctype = _CTYPE[a.split()[0]]
                assert c.__name__ == ctype or (ctype == "c_long" and c is ctypes.c_int64) or \
                    (ctype == "c_int" and c is ctypes.c_int32), (name, a, c)
        assert getattr(handle, name) is not None           # exported
    body = re.search(r"typedef struct xt_per_cfg \{(.*?)\} xt_per_cfg;", header, re.S).group(1)
    fields = [x.strip() for x in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if x.strip()]
    names, kinds = [], []
    for decl in fields:                                    # "const double* u" / "double alpha, beta, eps"
        _, rest = decl.replace("const ", "").split(None, 1)
        for n in rest.split(","):
            names.append(n.strip(" *"))
            kinds.append("*" in decl)
    assert names == [n for n, _ in L.PerCfg._fields_]
    for (n, ct), is_ptr in zip(L.PerCfg._fields_, kinds):
        assert (ct is ctypes.c_void_p) == is_ptr, n
    assert ctypes.sizeof(L.PerCfg) == 8 * 8 + 3 * 8
    # the uniform entries keep their shapes
    assert ctypes.sizeof(L.DqnCfg) == 40 and len(L.SIGNATURES["xt_dqn_loss"][1]) == 22
    assert len(L.SIGNATURES["xt_net_dqn_step"][1]) == 15


# ------------------------------------------------------------------------------------------------ configuration
class _NoStepModel(object):
    """a model with the reference's predict / train only"""

    def __init__(self, model_info):
        pass


class _FakeNet(object):
    inference_only = False
    device = "cpu"

    @staticmethod
    def to_device_obs(x):
        raise AssertionError("never reached")


class _StepModel(object):
    """claims the device step; nothing here runs it"""

    def __init__(self, model_info):
        self.net = _FakeNet()

    def train_replay(self, *a):
        raise AssertionError("never reached")

    train_replay_per = train_replay


def _alg(model, **cfg):
    from xingtian_amd.algorithm import alg_builder
    from xingtian_amd.register import Registers
    Registers.model._by_name[model.__name__] = model
    try:
        base = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1, "BUFFER_SIZE": 37, "BATCH_SIZE": 8}
        base.update(cfg)
        return alg_builder("DQN", {"actor": {"model_name": model.__name__, "state_dim": [3], "action_dim": 3}}, base)
    finally:
        del Registers.model._by_name[model.__name__]


def test_per_is_off_by_default_and_its_keys_parse_with_the_baselines_defaults():
    from xingtian_amd.algorithm.dqn.dqn import DeviceReplay, PrioritizedDeviceReplay
    alg = _alg(_StepModel)
    assert not alg.prioritized and type(alg.buff) is DeviceReplay
    alg = _alg(_StepModel, prioritized_replay=True)
    buf = alg.buff
    assert alg.prioritized and type(buf) is PrioritizedDeviceReplay
    assert (buf.alpha, buf.eps, buf.capacity, buf.cap2) == (0.6, 1e-6, 37, 64)
    assert alg.per_beta0 == 0.4 and alg.per_beta_iters is None
    for t in (0, 5, 10 ** 6):
        alg.train_count = t
        assert alg.per_beta() == 0.4                                       # None: constant
    alg = _alg(_StepModel, prioritized_replay=True, prioritized_replay_alpha=1.0, prioritized_replay_beta0=0.5,
               prioritized_replay_beta_iters=4, prioritized_replay_eps=1e-3)
    assert (alg.buff.alpha, alg.buff.eps) == (1.0, 1e-3)
    got = []
    for t in range(7):
        alg.train_count = t
        got.append(alg.per_beta())
    assert got == [0.5, 0.625, 0.75, 0.875, 1.0, 1.0, 1.0]                 # linear to 1.0 over 4 trains, then constant
    with pytest.raises(ValueError):
        _alg(_StepModel, prioritized_replay=True, prioritized_replay_beta0=0.0)
    with pytest.raises(ValueError):
        _alg(_StepModel, prioritized_replay=True, prioritized_replay_eps=0.0)
    with pytest.raises(ValueError):
        _alg(_StepModel, prioritized_replay=True, prioritized_replay_beta_iters=0)
    with pytest.raises(ValueError):
        _alg(_StepModel, prioritized_replay=True, BATCH_SIZE=1025)         # one thread per sample, one workgroup
    assert not _alg(_StepModel, BATCH_SIZE=1025).prioritized


def test_a_prioritised_train_on_fewer_than_two_transitions_raises_value_error():
    alg = _alg(_StepModel, prioritized_replay=True)
    with pytest.raises(ValueError) as info:
        alg.train()
    assert "at least 2" in str(info.value) and alg.train_count == 0


def test_per_is_refused_at_construction_on_a_model_without_the_device_step():
    with pytest.raises(NotImplementedError) as info:
        _alg(_NoStepModel, prioritized_replay=True)
    assert "prioritized_replay" in str(info.value) and "device step" in str(info.value)
    assert not _alg(_NoStepModel).prioritized                              # without the key it is built as before
    # the CPU replica of a real DQN model
    from xingtian_amd.algorithm import alg_builder
    info_d = {"actor": {"model_name": "DqnMlp", "state_dim": [4], "action_dim": 2,
                        "model_config": {"DEVICE": "cpu", "SEED": 1, "HIDDEN_SIZE": 8, "NUM_LAYERS": 1}}}
    cfg = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1, "BUFFER_SIZE": 10, "BATCH_SIZE": 4}
    with pytest.raises(NotImplementedError):
        alg_builder("DQN", info_d, dict(cfg, prioritized_replay=True))
    assert not alg_builder("DQN", info_d, cfg).device_step
