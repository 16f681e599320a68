"""CPU tests of the host side of the device-resident non-opt IMPALA train (``DEVICE_VTRACE``): the split of the host
v-trace, its float64 twin against the executed reference, the minibatch table and the shuffles of the device path, and
the ctypes prototypes of the two new C-ABI symbols."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# import_config overrides module globals for the rest of the process: restate what these tests rely on
MLP_CFG = {"NUM_LAYERS": 1, "HIDDEN_SIZE": 128, "LR": 3e-4, "ENTROPY_LOSS": 0.01, "SEED": 11, "DEVICE": "cpu"}


def _fixture_inputs():
    """the fragments of oracle/gen_golden_alg.py::impala_plain_inputs as [F, T, ...] arrays"""
    from oracle import gen_golden_alg as G
    msgs = G.impala_plain_inputs()
    t = G.IMPALA_PLAIN_CFG[1]["episode_len"]
    stack = lambda key: np.stack([np.asarray(m[key]) for m in msgs])
    return dict(t=t, onehot=stack("real_action"), behaviour=stack("action"), reward=stack("reward").reshape(2, t, 1),
                done=stack("done").reshape(2, t, 1))


def _seeded_case(f=5, t=128, a=6, seed=71):
    rng = np.random.default_rng(seed)
    soft = lambda x: np.exp(x) / np.exp(x).sum(-1, keepdims=True)
    value = rng.standard_normal((f, t + 1, 1)).astype(np.float32)
    return dict(target_prob=soft(rng.standard_normal((f, t, a))).astype(np.float32),
                behaviour_prob=soft(rng.standard_normal((f, t, a))).astype(np.float32),
                onehot=np.eye(a, dtype=np.float32)[rng.integers(0, a, (f, t))],
                reward=rng.choice([-1.0, 0.0, 1.0], (f, t, 1)), done=rng.random((f, t, 1)) < 0.05,
                value=value[:, :-1], value_next=value[:, 1:], gamma=0.99)


def test_rho_plus_recursion_equals_the_whole_host_vtrace(golden_dir):
    from xingtian_amd.algorithm.impala.impala import rho_from_probs, vtrace_from_probs, vtrace_from_rho
    z = np.load(os.path.join(golden_dir, "alg_impala.npz"))
    fx = _fixture_inputs()
    t = fx["t"]
    p, v = z["pred_p"].reshape(2, t + 1, -1), z["pred_v"].reshape(2, t + 1, 1)
    cases = [dict(target_prob=p[:, :-1], behaviour_prob=fx["behaviour"], onehot=fx["onehot"], reward=fx["reward"],
                  done=fx["done"], value=v[:, :-1], value_next=v[:, 1:], gamma=0.99), _seeded_case()]
    for c in cases:
        whole = vtrace_from_probs(**c)
        rho = rho_from_probs(c["target_prob"], c["behaviour_prob"], c["onehot"])
        assert rho.shape == c["reward"].shape and rho.max() <= 1.0 and (rho < 1.0).any()
        split = vtrace_from_rho(rho, c["reward"], c["done"], c["value"], c["value_next"], c["gamma"])
        assert np.array_equal(whole[0], split[0]) and np.array_equal(whole[1], split[1])
        assert whole[0].dtype == np.float64 and whole[0].shape == c["reward"].shape


def test_float64_twin_stays_within_1e6_of_the_executed_reference(golden_dir):
    """The twin (every input cast to float64) against the pg_adv / target the EXECUTED reference handed to its model
    (tests/golden/alg_impala.npz).  The reference takes its logs in float32 (probabilities and one-hots arrive as
    float32): 1e-6 absolute is a convention check, not a precision claim (observed 3.6e-8 / 3.7e-8)."""
    from xingtian_amd.algorithm.impala.impala import vtrace_from_probs
    z = np.load(os.path.join(golden_dir, "alg_impala.npz"))
    fx = _fixture_inputs()
    t = fx["t"]
    f64 = lambda x: np.asarray(x, dtype=np.float64)
    p, v = f64(z["pred_p"]).reshape(2, t + 1, -1), f64(z["pred_v"]).reshape(2, t + 1, 1)
    pg, tgt = vtrace_from_probs(p[:, :-1], f64(fx["behaviour"]), f64(fx["onehot"]), f64(fx["reward"]), fx["done"],
                                v[:, :-1], v[:, 1:], 0.99)
    ref_pg = np.concatenate([z["train_%d_state_1" % i] for i in range(int(z["train_ncalls"]))])
    ref_tgt = np.concatenate([z["train_%d_label_1" % i] for i in range(int(z["train_ncalls"]))])
    d_pg, d_tgt = np.abs(pg.reshape(-1, 1) - ref_pg).max(), np.abs(tgt.reshape(-1, 1) - ref_tgt).max()
    print("twin vs executed reference: pg_adv %.3g target %.3g" % (d_pg, d_tgt))
    assert d_pg <= 1e-6 and d_tgt <= 1e-6


def _host_path_fit_calls(n, batch_size, frags, seed):
    """(rows, order) of every ``fit_in_order`` call that IMPALA.train -> model.train makes, on a CPU-built model"""
    from xingtian_amd.algorithm import alg_builder
    t = n // frags
    alg = alg_builder("IMPALA", {"actor": {"model_name": "ImpalaMlp", "state_dim": [4], "action_dim": 2,
                                           "model_config": dict(MLP_CFG)}},
                      {"instance_num": frags, "agent_num": 1, "prepare_times_per_train": frags, "BATCH_SIZE": batch_size,
                       "episode_len": t, "GAMMA": 0.99})
    calls = []

    def fit_in_order(obs, adv, onehot, target, order):
        assert len(obs) == len(adv) == len(onehot) == len(target) == len(order)
        calls.append((len(obs), np.array(order, copy=True)))
        return 0.25

    alg.actor.fit_in_order = fit_in_order
    rng = np.random.default_rng(5)
    for _ in range(frags):
        alg.prepare_data({"cur_state": rng.uniform(-1, 1, (t + 1, 4)).astype(np.float32),
                          "real_action": np.eye(2, dtype=np.float32)[rng.integers(0, 2, t)],
                          "reward": [1.0] * t, "done": [False] * t, "action": np.full((t, 2), 0.5, np.float32)})
    np.random.seed(seed)
    assert alg.train() == 0.25
    return calls


@pytest.mark.parametrize("n,batch_size,frags", [(40, 16, 2), (150, 200, 3), (400, 800, 2), (300, 128, 3)])
def test_minibatch_table_and_shuffles_equal_the_host_path(n, batch_size, frags):
    from xingtian_amd.model.hip_net import keras_fit_table, keras_lr_t
    from xingtian_amd.model.impala.impala_cnn import FIT_BATCH, draw_fit_orders
    calls = _host_path_fit_calls(n, batch_size, frags, seed=123)
    assert sum(rows for rows, _ in calls) == n
    expect = []                                   # (offset, rows, chunk) as fit_in_order walks every recorded call
    lo = 0
    for chunk, (rows, _) in enumerate(calls):
        for m in range(0, rows, FIT_BATCH):
            expect.append((lo + m, min(FIT_BATCH, rows - m), chunk))
        lo += rows
    for decay in (0.0, 0.05):
        for iterations in (0, 7):
            table = keras_fit_table(n, batch_size, FIT_BATCH, iterations, 3e-4, decay)
            assert [e[:3] for e in table] == expect
            assert all(1 <= e[1] <= 128 for e in table)
            for k, e in enumerate(table):
                assert e[3] == float(keras_lr_t(3e-4, iterations + k, decay)) and isinstance(e[3], float)
    # the same seed draws the same permutations, chunk by chunk
    np.random.seed(123)
    orders = draw_fit_orders(n, batch_size)
    assert len(orders) == len(calls)
    for o, (rows, ref) in zip(orders, calls):
        assert len(o) == rows and np.array_equal(o, ref)
    assert any(not np.array_equal(o, np.arange(len(o))) for o in orders)


@pytest.mark.parametrize("decay", [0.0, 0.05])
@pytest.mark.parametrize("iterations", [0, 7])
def test_factored_lr_t_is_the_adam_keras_formula(decay, iterations):
    """``keras_lr_t`` against the formula as ``HipActorCritic.adam_keras`` spelled it out before the factoring."""
    from xingtian_amd.model.hip_net import keras_lr_t
    lr, beta1, beta2 = 3e-4, 0.9, 0.999
    t = iterations + 1
    ref = np.float32(lr) / (np.float32(1.0) + np.float32(decay) * np.float32(iterations))
    ref = ref * np.sqrt(np.float32(1.0) - np.float32(beta2) ** t) / (np.float32(1.0) - np.float32(beta1) ** t)
    got = keras_lr_t(lr, iterations, decay)
    assert float(got) == float(ref) and np.asarray(got).dtype == np.asarray(ref).dtype


def test_header_and_signatures_list_the_new_symbols():
    from xingtian_amd import lib
    header = open(os.path.join(ROOT, "include", "xt_mi355x.h")).read()
    declared = set(re.findall(r"\b(xt_[a-z0-9_]+)\s*\(", header))
    for name, nargs in (("xt_vtrace_probs_f64", 15), ("xt_net_keras_impala_train", 21)):
        assert name in declared and name in lib.SIGNATURES
        assert len(lib.SIGNATURES[name][1]) == nargs
        assert hasattr(lib.load(), name)
    assert lib.load().xt_abi_version() == 12
    import ctypes
    assert ctypes.sizeof(lib.KerasFitEntry) == 16 and ctypes.sizeof(lib.KerasTrainCfg) == 64
