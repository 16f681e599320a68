"""CPU checks of the per-update PPO training diagnostics (``model_config.TRAIN_STATS``): the host derivation of the
dict from the 16 device sums, the agreement of the header's slot macros with ``xingtian_amd.lib``, and the CPU replica,
which reads the same configuration and ignores the key."""
import math
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hand_sums():
    """two steps over 3 + 1 rows, every slot a value that is exact in binary"""
    a = np.zeros(16)
    a[0], a[1] = 2.0, 4.0                    # steps, rows
    a[2], a[3], a[4] = -0.5, 3.0, 0.25       # sum of the steps' surrogate / entropy / critic-loss means
    a[5], a[6], a[7] = 0.125, 1.0, 3.0       # sum(old_logp - logp), rows clipped, rows value-clipped
    tv = np.array([1.0, 2.0, 3.0, 6.0])
    err = np.array([0.5, -0.5, 1.5, 0.5])    # tv - v
    a[8], a[9], a[10], a[11] = tv.sum(), (tv * tv).sum(), err.sum(), (err * err).sum()
    a[12], a[13], a[14] = 3.0, 2.5, 1.0      # sum / max of the gradient norm, steps clipped
    return a, tv, err


def test_hand_made_sums_give_the_hand_computed_dict():
    from xingtian_amd.ops import ppo_stats_from_sums
    a, tv, err = hand_sums()
    d = ppo_stats_from_sums(a, ent_coef=0.5, critic_coef=2.0)
    assert set(d) == {"loss", "policy_loss", "entropy", "value_loss", "approx_kl", "clip_fraction", "vf_clip_fraction",
                      "explained_variance", "grad_norm", "grad_norm_max", "grad_clip_fraction", "steps", "rows"}
    assert all(type(v) is float for v in d.values())
    assert d["steps"] == 2.0 and d["rows"] == 4.0
    assert d["policy_loss"] == 0.25 and d["entropy"] == 1.5 and d["value_loss"] == 0.125
    assert d["loss"] == 0.25 - 0.5 * 1.5 + 2.0 * 0.125            # derived when the caller has no loss to hand in
    assert d["approx_kl"] == 0.125 / 4 and d["clip_fraction"] == 0.25 and d["vf_clip_fraction"] == 0.75
    assert d["grad_norm"] == 1.5 and d["grad_norm_max"] == 2.5 and d["grad_clip_fraction"] == 0.5
    # Var(tv) = 3.5, Var(tv - v) = 0.5 (population variances): 1 - 0.5 / 3.5
    assert tv.var() == 3.5 and err.var() == 0.5
    assert abs(d["explained_variance"] - (1.0 - 0.5 / 3.5)) < 1e-15
    # the loss Model.train returned is handed through untouched
    assert ppo_stats_from_sums(a, loss=float(np.float32(0.3)))["loss"] == float(np.float32(0.3))
    assert ppo_stats_from_sums(list(a))["policy_loss"] == 0.25                  # any sequence of 16


def test_constant_targets_give_nan_and_no_steps_give_none():
    from xingtian_amd.ops import ppo_stats_from_sums
    a, _, _ = hand_sums()
    tv = np.float64(np.float32(0.7))          # the same fp32 target on every row: Var(tv) == 0
    a[8], a[9] = 4 * tv, 4 * tv * tv
    d = ppo_stats_from_sums(a)
    assert math.isnan(d["explained_variance"]) and d["approx_kl"] == 0.125 / 4
    z = np.zeros(16)
    assert ppo_stats_from_sums(z) is None
    a[0] = 0.0
    assert ppo_stats_from_sums(a) is None
    try:
        ppo_stats_from_sums(np.zeros(15))
    except ValueError:
        pass
    else:
        raise AssertionError("15 sums were accepted")


def test_header_macros_and_lib_agree_on_the_sixteen_slots():
    from xingtian_amd import lib
    header = open(os.path.join(ROOT, "include", "xt_mi355x.h")).read()
    macros = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+XT_TRAIN_STATS_([A-Z_]+)\s+(\d+)", header)}
    assert macros.pop("DOUBLES") == lib.TRAIN_STATS_DOUBLES == 16
    assert macros == lib.TRAIN_STATS_SLOTS
    assert sorted(macros.values()) == list(range(16))
    assert (macros["STEPS"], macros["ROWS"], macros["KL"], macros["GNORM_MAX"], macros["RESERVED"]) == (0, 1, 5, 13, 15)
    heads = {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define\s+XT_NET_HEAD_([A-Z]+)\s+(0x[0-9a-fA-F]+)", header)}
    assert heads == {"PLAIN": lib.NET_HEAD_PLAIN, "GAUSS": lib.NET_HEAD_GAUSS}
    assert re.search(r"\bint\s+xt_net_set_train_stats\s*\(\s*xt_net\s*\*\s*net,\s*double\s*\*\s*stats,\s*float\s*\*\s*rows\s*\)\s*;",
                     header)
    res, args = lib.SIGNATURES["xt_net_set_train_stats"]
    assert res is lib.c_int32 and len(args) == 3
    assert lib.SIGNATURES["xt_net_last_head_path"] == (lib.c_int32, [lib.c_void_p])
    h = lib.load()
    assert hasattr(h, "xt_net_set_train_stats") and hasattr(h, "xt_net_last_head_path")
    assert h.xt_abi_version() == 12
    # refused before any device call: a null net
    assert h.xt_net_set_train_stats(None, None, None) != 0 and b"xt_net_set_train_stats" in h.xt_last_error()


def test_cpu_replica_ignores_the_key():
    from xingtian_amd.algorithm import alg_builder
    from xingtian_amd.model import model_builder
    for name, extra in (("PpoMlp", {"state_dim": [8], "action_dim": 4}),
                        ("PpoMlp", {"state_dim": [3], "action_dim": 3, "action_type": "DiagGaussian"})):
        cfg = {"TRAIN_STATS": True, "SEED": 1, "DEVICE": "cpu"}
        if "action_type" in extra:
            cfg["action_type"] = extra["action_type"]
        info = {"model_name": name, "state_dim": extra["state_dim"], "action_dim": extra["action_dim"], "model_config": cfg}
        model = model_builder(info)
        assert model.net.inference_only
        action, logp, value = model.predict(np.zeros((5,) + tuple(extra["state_dim"]), np.float32))
        assert len(action) == 5 and logp.shape == (5, 1) and value.shape == (5, 1)
        assert model.train_stats() is None
    alg = alg_builder("PPO", {"actor": {"model_name": "PpoMlp", "state_dim": [8], "action_dim": 4,
                                        "model_config": {"TRAIN_STATS": True, "DEVICE": "cpu"}}},
                      {"instance_num": 1, "agent_num": 1})
    assert alg.train_stats() is None
