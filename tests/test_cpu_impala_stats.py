"""CPU checks of the per-train IMPALA v-trace diagnostics (``ImpalaCnnOpt`` ``model_config.TRAIN_STATS``): the host
derivation of the dict from the 16 device sums, the agreement of the header's macros with ``xingtian_amd.lib``, the input
recipe and the float64 restatement of tests/impala_stats_helpers.py (tied to ``oracle.nets.impala_loss_and_grads``), the
configurations that are refused, and the CPU replica, which reads the same configuration and ignores the key."""
import math
import os
import re

import numpy as np
import pytest

import impala_stats_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"chunks", "transitions", "behaviour_kl", "rho_mean", "rho_max", "rho_clip_fraction", "entropy", "pg_loss",
        "baseline_loss", "entropy_loss", "explained_variance", "vs_mean", "grad_norm", "grad_norm_max", "grad_clip_fraction",
        "loss"}


def hand_sums():
    """two chunks over 3 + 1 transitions, every slot a value that is exact in binary"""
    a = np.zeros(16)
    vs = np.array([1.0, 2.0, 3.0, 6.0])
    err = np.array([0.5, -0.5, 1.5, 0.5])          # vs - v
    a[0], a[1] = 2.0, 4.0                          # chunks, transitions
    a[2], a[3] = -3.0, 5.0                         # sum ce * pg, sum entropy
    a[4], a[5], a[6], a[7] = (err * err).sum(), err.sum(), vs.sum(), (vs * vs).sum()
    a[8], a[9], a[10], a[11] = 0.5, 4.5, 1.0, 2.25     # sum -log rho, sum rho, rho > 1, max rho
    a[12], a[13], a[14] = 3.0, 2.5, 1.0            # sum / max of the gradient norm, chunks clipped
    return a, vs, err


def test_hand_made_sums_give_the_hand_computed_dict():
    from xingtian_amd.ops import impala_stats_from_sums
    a, vs, err = hand_sums()
    d = impala_stats_from_sums(a)
    assert set(d) == KEYS and all(type(v) is float for v in d.values())
    assert d["chunks"] == 2.0 and d["transitions"] == 4.0
    assert d["behaviour_kl"] == 0.125 and d["rho_mean"] == 1.125 and d["rho_max"] == 2.25 and d["rho_clip_fraction"] == 0.25
    assert d["entropy"] == 1.25 and d["vs_mean"] == 3.0
    assert d["pg_loss"] == -1.5 and d["baseline_loss"] == 0.5 * 3.0 / 2 and d["entropy_loss"] == -2.5
    assert d["grad_norm"] == 1.5 and d["grad_norm_max"] == 2.5 and d["grad_clip_fraction"] == 0.5
    assert vs.var() == 3.5 and err.var() == 0.5                # population variances
    assert abs(d["explained_variance"] - (1.0 - 0.5 / 3.5)) < 1e-15
    # the recombination identity, with the kernel's own constants; the caller's loss is handed through untouched
    assert d["loss"] == d["pg_loss"] + 0.5 * d["baseline_loss"] + 0.01 * d["entropy_loss"]
    assert impala_stats_from_sums(a, loss=float(np.float32(0.3)))["loss"] == float(np.float32(0.3))
    assert impala_stats_from_sums(list(a))["pg_loss"] == -1.5                   # any sequence of 16


def test_zero_chunks_give_none_and_constant_targets_nan():
    from xingtian_amd.ops import impala_stats_from_sums
    assert impala_stats_from_sums(np.zeros(16)) is None
    a, _, _ = hand_sums()
    vs = np.float64(np.float32(0.7))
    a[6], a[7] = 4 * vs, 4 * vs * vs               # the same fp32 target on every transition: Var(vs) == 0
    d = impala_stats_from_sums(a)
    assert math.isnan(d["explained_variance"]) and d["behaviour_kl"] == 0.125
    a[0] = 0.0
    assert impala_stats_from_sums(a) is None
    with pytest.raises(ValueError):
        impala_stats_from_sums(np.zeros(15))


def test_header_macros_lib_constants_and_signatures_agree():
    from xingtian_amd import lib
    header = open(os.path.join(ROOT, "include", "xt_mi355x.h")).read()
    macros = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+XT_IMPALA_STATS_([A-Z_]+)\s+(\d+)", header)}
    assert macros.pop("DOUBLES") == lib.IMPALA_STATS_DOUBLES == 16
    assert macros == lib.IMPALA_STATS_SLOTS and sorted(macros.values()) == list(range(16))
    assert re.search(r"#define\s+XT_IMPALA_TRAJ_STATS_FLOATS\s+12\b", header) and lib.IMPALA_TRAJ_STATS_FLOATS == 12 == H.K
    assert re.search(r"#define\s+XT_IMPALA_PATH_LOSS\s+3\b", header) and lib.IMPALA_PATH_LOSS == 3
    assert re.search(r"#define\s+XT_IMPALA_PATH_STATS_BIT\s+0x10000\b", header) and lib.IMPALA_PATH_STATS_BIT == 0x10000
    # column c of a trajectory row feeds slot PG + c
    order = ["PG", "ENT", "VERR_SQ", "VERR", "VS", "VS_SQ", "NEG_LOG_RHO", "RHO", "RHO_CLIPPED", "RHO_MAX"]
    assert [macros[k] for k in order] == list(range(2, 12)) and len(H.COLUMNS) == 10 and H.MAX_COL == 9
    # the gradient-norm slots are those of the PPO statistics (one device helper serves both)
    for k in ("GNORM_SUM", "GNORM_MAX", "GNORM_CLIPPED"):
        assert macros[k] == lib.TRAIN_STATS_SLOTS[k]
    assert re.search(r"\bint\s+xt_net_set_impala_stats\s*\(\s*xt_net\s*\*\s*net,\s*double\s*\*\s*stats,\s*float\s*\*\s*"
                     r"traj_stats,\s*int32_t\s+max_traj\s*\)\s*;", header)
    assert lib.SIGNATURES["xt_net_set_impala_stats"] == (lib.c_int32, [lib.c_void_p, lib.c_void_p, lib.c_void_p, lib.c_int32])
    # the stats entries take the arguments of the existing ones, plus traj_stats, stats (and the loss entry's path_out)
    res, args = lib.SIGNATURES["xt_impala_heads_stats_ex"]
    assert (res, args[:-2]) == lib.SIGNATURES["xt_impala_heads_ex"] and args[-2:] == [lib.c_void_p, lib.c_void_p]
    res, args = lib.SIGNATURES["xt_impala_loss_stats"]
    assert (res, args[:-3]) == lib.SIGNATURES["xt_impala_loss"] and args[-3:-1] == [lib.c_void_p, lib.c_void_p]
    h = lib.load()
    for name in ("xt_net_set_impala_stats", "xt_impala_heads_stats_ex", "xt_impala_loss_stats"):
        assert hasattr(h, name)
    assert h.xt_abi_version() == 12
    # refused before any device call: a null net
    assert h.xt_net_set_impala_stats(None, None, None, 0) != 0 and b"xt_net_set_impala_stats" in h.xt_last_error()


@pytest.mark.parametrize("case", H.CASES, ids=["x".join(map(str, c)) for c in H.CASES])
def test_recipe_margin_and_restatement_against_the_oracle(case):
    from oracle import nets
    n_traj, T, A = case
    d = H.make_inputs(*case)                       # (asserts the margin itself)
    print("impala_stats recipe: case %s margin %.3e on-policy %d done %d" % (case, d["margin"], int(d["on_policy"].sum()),
                                                                           int(d["done"].sum())))
    assert d["margin"] >= H.MARGIN
    assert np.array_equal(d["bp"][d["on_policy"]].view(np.uint32), d["logits"][d["on_policy"]].view(np.uint32))
    assert (np.abs(d["reward"]) > 1.0).any() or n_traj * T < 8                 # the reward clip acts
    r = H.restate(d["logits"], d["baseline"], d["bp"], d["action"], d["done"], d["reward"], T)
    loss, _, _, parts = nets.impala_loss_and_grads(d["logits"], d["baseline"], d["bp"], d["action"], d["done"], d["reward"],
                                                   T, H.GAMMA, np.float64)
    mine = r["terms"].sum()
    assert abs(mine - loss) <= 1e-12 * abs(loss), (case, mine, loss)
    assert np.allclose(r["vs"], np.swapaxes(parts["vs"], 0, 1), rtol=1e-12, atol=1e-12)
    assert np.allclose(r["pg"], np.swapaxes(parts["pg_adv"], 0, 1), rtol=1e-12, atol=1e-12)
    # on-policy transitions: rho == 1 exactly, not counted as clipped
    on = d["on_policy"].reshape(n_traj, T)[:, :-1]
    assert (r["rho"][on] == 1.0).all() and (r["clipped"][on] == 0.0).all() and (r["neg_log_rho"][on] == 0.0).all()
    want, mag = H.sums16([r])
    assert want[0] == 1.0 and want[1] == n_traj * (T - 1) and want[10] == (r["rho"] > 1.0).sum()
    assert abs(want[2] + 0.5 * 0.5 * want[4] - 0.01 * want[3] - loss) <= 1e-12 * abs(loss)


def info(**cfg):
    return {"model_name": "ImpalaCnnOpt", "state_dim": [42, 42, 4], "action_dim": 6, "input_dtype": "uint8",
            "model_config": dict(cfg)}


def test_refused_configurations_raise_value_error(monkeypatch):
    from xingtian_amd.model import model_builder
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(ValueError, match="ASYNC_LOSS"):
        model_builder(info(TRAIN_STATS=True, ASYNC_LOSS=True))
    for mode in ("strict", "weak"):
        with pytest.raises(ValueError, match="TRAIN_STATS"):
            model_builder(info(TRAIN_STATS=True, DP=mode))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="WORLD_SIZE"):
        model_builder(info(TRAIN_STATS=True))


def test_cpu_replica_ignores_the_key():
    from xingtian_amd.algorithm import alg_builder
    from xingtian_amd.model import model_builder
    model = model_builder(info(TRAIN_STATS=True, SEED=1, DEVICE="cpu"))
    assert model.net.inference_only
    logits, value, action = model.predict(np.zeros((3, 42, 42, 4), np.uint8))
    assert np.asarray(logits).shape == (3, 6) and len(action) == 3
    assert model.train_stats() is None
    alg = alg_builder("IMPALAOpt", {"actor": info(TRAIN_STATS=True, DEVICE="cpu")}, {"instance_num": 1, "agent_num": 1})
    assert alg.train_stats() is None
