"""Time one SCC train (xt_scc_step + xt_scc_apply) on the device at the shipped example's shape and at a five-agent two-group
one, and the same train, masked critic passes included, written in eager PyTorch on the same device (the outside-HIP
alternative).  Device events around work that is already on the device; warm-up first; medians with their spread.

    python tools/scc_probe.py [--reps 20] [--out scc_probe.json]
"""
import argparse
import ctypes
import json
import os
import random
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import qmix_helpers as Q                                   # noqa: E402  (the agent, restated in torch)
from tests import scc_helpers as S                                    # noqa: E402  (the critic and the credit loops)
from tools.qmix_probe import timed                                    # noqa: E402
from xingtian_amd import lib as L                                      # noqa: E402
from xingtian_amd.model.scc.scc_model import HipScc                    # noqa: E402

BASE = dict(rnn_hidden_dim=64, dense_unit_number=128, enable_critic_multi_channel=True, channel_merge="concat", batch_size=32,
            episode_limit=300)
SHAPES = {
    "example (2s_vs_1sc: B 32, n 2, o + A 24, U 128, 301 steps)": dict(n_agents=2, obs_shape=26, n_actions=7, map_name="2s_vs_1sc"),
    "five agents, groups [2, 3] (B 32, o + A 24, U 128, 301 steps)": dict(n_agents=5, obs_shape=29, n_actions=7, map_name="2s3z"),
}


def launches(groups):
    """of one train, counted from the call sequence of xt_scc_step / xt_scc_apply: critic 5 (pass, sum(mask), TD, loss, backward),
    4 per group and 2 for the final Dense (weight gradients), agent's forward 5, actor head 2, agent's backward 16, optimisers 5"""
    return 5 + 4 * groups + 2 + 5 + 2 + 16 + 5


def eager_step(spec, case, p, slots, step, mc_times=3, gamma=0.99, lr=0.0005, clip=10.0):
    """the same train in eager PyTorch (float32, autograd): the reference's 2 n K (or 2 n) masked critic passes, both losses, both
    optimisers with per-tensor clipping"""
    x = case["x"]
    with torch.no_grad():
        credits = S.credits_ref(spec, lambda y: S.critic_ref(spec, p, "eval_mixer", y), x, mc_times, random.Random(step))
    v = S.critic_ref(spec, p, "eval_mixer", x)
    y = case["rewards"] + gamma * (1.0 - case["terminated"]) * S.critic_ref(spec, p, "target_mixer", x).detach()
    mixer = (((v - y) * case["mask"]) ** 2).sum() / case["mask"].sum()
    q, _ = Q.agent_ref(p, "eval_agent", case["traj"], case["lens"], case["h0"])
    chosen = (q[:, :-1] * case["onehot"]).sum(-1)
    alive = case["mask"].repeat(1, 1, spec.n)
    actor = ((chosen * alive - credits * alive) ** 2).sum() / alive.sum()
    ev = [k for k in p if k.startswith("eval")]
    grads = torch.autograd.grad(actor + mixer, [p[k] for k in ev])
    alpha = lr * np.sqrt(1 - 0.999 ** (step + 1)) / (1 - 0.9 ** (step + 1))
    with torch.no_grad():
        for k, g in zip(ev, grads):
            g = g * clip / torch.clamp(g.norm(), min=clip)
            if k.startswith("eval_agent"):
                ms, = slots[k]
                ms += (g * g - ms) * 0.1
                p[k] -= lr * g / torch.sqrt(ms + 1e-10)
            else:
                m, v2 = slots[k]
                m += (g - m) * 0.1
                v2 += (g * g - v2) * 0.001
                p[k] -= alpha * m / (torch.sqrt(v2) + 1e-8)
    return actor + mixer


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--eager-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L.require_gpu()
    lib = L.load()
    report = dict(device=torch.cuda.get_device_name(0), kernel_sources_sha=L.kernel_sources_sha())
    for name, dims in SHAPES.items():
        spec = S.SCCSpec(dict(BASE, **dims))
        net = HipScc(spec, seed=0)
        case = S.make_case(spec, 32, 7)
        a = S.train_args(case)
        net.grad_step(a[0], a[1], a[2], a[4], *a[7:])      # stages the batch on the device (net._keep)
        ptrs = [L.ptr(x) for x in net._keep]

        def hip_train():
            L.check(lib.xt_scc_step(net.handle, *ptrs, 32, ctypes.byref(net.cfg), L.ptr(net.loss_dev), L.stream_ptr()), "step")
            L.check(lib.xt_scc_apply(net.handle, ctypes.byref(net.cfg), L.stream_ptr()), "apply")

        row = dict(launches_per_train=launches(len(spec.groups)), hip_train=timed(hip_train, args.reps))
        dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()      # noqa: E731
        ecase = dict(x=dev(S.critic_state(spec, case["obs"], case["actions"]).astype(np.float32)), traj=dev(case["traj"]),
                     lens=dev(np.asarray(case["lens"]).astype(np.int64)), h0=torch.zeros(32 * spec.n, spec.H, device="cuda"),
                     onehot=torch.nn.functional.one_hot(dev(case["actions"][..., 0].astype(np.int64)), spec.A).float(),
                     rewards=dev(case["rewards"]), terminated=dev(case["terminated"]), mask=dev(case["mask"]))
        p = {k: dev(v).requires_grad_(k.startswith("eval")) for k, v in S.make_params(spec, 1).items()}
        slots = {k: [torch.ones_like(v)] if k.startswith("eval_agent") else [torch.zeros_like(v), torch.zeros_like(v)]
                 for k, v in p.items() if k.startswith("eval")}
        row["eager_train"] = timed(lambda: eager_step(spec, ecase, p, slots, 0), args.eager_reps, warm=2)
        report[name] = row
        print(name, json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
