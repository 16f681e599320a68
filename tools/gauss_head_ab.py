#!/usr/bin/env python
"""A/B of the fused DiagGaussian PPO head (model_config.GAUSS_FUSED_HEAD / xt_net_set_gauss_fused) against the default
three launches, in ONE process with the two arms alternating; GPU box.

    python tools/gauss_head_ab.py [--rounds 7] [--reps 20] [--out profiles/gauss_fused_head.json]
    python tools/gauss_head_ab.py --trace off|on --workload a|b      # a few replays of ONE arm, for rocprofv3 --kernel-trace

Workloads (HBM-resident rollout of 4096 rows x 4 epochs, whole xt_net_ppo_train graph replays, device-synchronised wall time):
  a  examples/pendulum_ppo.yaml's network: PpoMlp (3,) -> tanh 64-64, separate trunks, A = 1, BATCH_SIZE 200
  b  a DiagGaussian PpoCnn [84, 84, 3] uint8, hidden [256], A = 8, BATCH_SIZE 320
Per workload and arm: median and range of the per-update time over the rounds (each round = `reps` replays of one arm, the
arms taking turns), and the plugin-path updates/s of workload a with STREAM_INGEST false and true (prepare_data + train)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xingtian_amd.model import netspec  # noqa: E402
from xingtian_amd.model.hip_net import HipActorCritic  # noqa: E402

N, EPOCHS = 4096, 4
PENDULUM = dict(BATCH_SIZE=200, CRITIC_LOSS_COEF=1.0, ENTROPY_LOSS=0.01, LR=0.0003, LOSS_CLIPPING=0.2, MAX_GRAD_NORM=5.0,
                NUM_SGD_ITER=EPOCHS, VF_CLIP=10.0)      # examples/pendulum_ppo.yaml:26-37 (NUM_SGD_ITER: the A/B's 4 epochs)
WORKLOADS = {
    "a": dict(spec=lambda: netspec.ppo_mlp((3,), 1, (64, 64), "tanh", False, action_type="DiagGaussian"), batch=200, a_dim=1,
              obs=lambda rng: rng.uniform(-1, 1, (N, 4)).astype(np.float32)),       # (3 columns + the zero column of netspec._mlp)
    "b": dict(spec=lambda: netspec.ppo_cnn((84, 84, 3), 8, (256,), "relu", True, action_type="DiagGaussian"), batch=320,
              a_dim=8, obs=lambda rng: rng.integers(0, 256, (N, 84, 84, 4)).astype(np.uint8)),
}


def make_arm(name, fused):
    w = WORKLOADS[name]
    dev = torch.device("cuda", 0)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.default_rng(0)
    obs = w["obs"](rng)
    if name == "a":
        obs[:, 3] = 0.0
    net = HipActorCritic(w["spec"](), max_batch=w["batch"], seed=0)
    if fused:
        net.set_gauss_fused(True)
    cfg = net.make_ppo_cfg(dict(PENDULUM, BATCH_SIZE=w["batch"]))
    data = (d(obs), d(np.stack([rng.permutation(N) for _ in range(EPOCHS)]).astype(np.int32)),
            d(rng.standard_normal((N, w["a_dim"])).astype(np.float32)),
            d((-np.abs(rng.standard_normal(N)) - 0.5).astype(np.float32)), d(rng.standard_normal(N)),
            d(rng.standard_normal(N).astype(np.float32)), d(rng.standard_normal(N)))
    return net, cfg, data


def replay(arm, reps):
    net, cfg, data = arm
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        net.ppo_train(cfg, *data, use_graph=True)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / reps


def ab(name, rounds, reps):
    arms = {"off": make_arm(name, False), "on": make_arm(name, True)}
    for arm in arms.values():
        replay(arm, 3)                                  # capture + warm-up
    ms = {"off": [], "on": []}
    for _ in range(rounds):                             # the arms take turns: drift hits both alike
        for k in ("off", "on"):
            ms[k].append(replay(arms[k], reps))
    steps = EPOCHS * -(-N // WORKLOADS[name]["batch"])
    out = {"workload": name, "steps_per_update": steps, "rounds": rounds, "reps": reps}
    for k, v in ms.items():
        out[k] = {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)),
                  "us_per_step": 1e3 * float(np.median(v)) / steps, "head_path": hex(arms[k][0].last_head_path())}
    out["delta_us_per_step"] = out["on"]["us_per_step"] - out["off"]["us_per_step"]
    return out


def host_path(stream, updates=12):
    """plugin-path updates/s of workload a: 32 trajectories of 128 steps through prepare_data, then train"""
    from xingtian_amd.algorithm import alg_builder
    cfg = dict(PENDULUM, VF_SHARE_LAYERS=False, activation="tanh", hidden_sizes=[64, 64], action_type="DiagGaussian", SEED=0,
               STREAM_INGEST=stream)
    alg = alg_builder("PPO", {"actor": {"model_name": "PpoMlp", "state_dim": [3], "action_dim": 1, "input_dtype": "float32",
                                        "model_config": cfg}}, {"instance_num": 32, "agent_num": 1})
    rng = np.random.default_rng(1)
    trajs = [dict(cur_state=rng.uniform(-1, 1, (128, 3)).astype(np.float32), action=rng.standard_normal((128, 1)).astype(np.float32),
                  logp=(-np.abs(rng.standard_normal((128, 1))) - 0.5).astype(np.float32), adv=rng.standard_normal((128, 1)),
                  old_value=rng.standard_normal((128, 1)).astype(np.float32), target_value=rng.standard_normal((128, 1)))
             for _ in range(32)]
    t0 = None
    for u in range(updates + 3):
        if u == 3:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
        for tr in trajs:
            alg.prepare_data(dict(tr))
        alg.train()
    torch.cuda.synchronize()
    return updates / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", choices=["off", "on"], default=None)
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default=None)
    args = ap.parse_args()
    if args.rounds < 5:
        raise SystemExit("at least 5 alternations")
    if args.trace:
        arm = make_arm(args.workload or "a", args.trace == "on")
        replay(arm, 5)
        print("traced arm", args.trace, "workload", args.workload or "a", "head path", hex(arm[0].last_head_path()))
        return
    res = {"ab": [ab(k, args.rounds, args.reps) for k in sorted(WORKLOADS) if args.workload in (None, k)]}
    if args.workload in (None, "a"):
        res["host_path_updates_per_s"] = {"STREAM_INGEST_false": host_path(False), "STREAM_INGEST_true": host_path(True)}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
