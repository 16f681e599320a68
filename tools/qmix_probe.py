"""Time one QMIX train (xt_qmix_step + xt_qmix_apply) on the device at the shipped example's shape and at a wide one, the two
persistent recurrent kernels stand-alone, and the same step written in eager PyTorch on the same device (the outside-HIP
alternative).  Device events around work that is already on the device; warm-up first; medians with their spread.

    python tools/qmix_probe.py [--reps 20] [--out qmix_probe.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import qmix_helpers as Q                                   # noqa: E402  (the graph, restated in torch)
from xingtian_amd import lib as L                                      # noqa: E402
from xingtian_amd.model.qmix.qmix_model import HipQmix, QMixSpec       # noqa: E402

SHAPES = {
    "example (2s_vs_1sc: B 32, n 2, seq_len 300)": dict(n_agents=2, obs_shape=26, n_actions=7, state_shape=27, episode_limit=300),
    "wide (27m_vs_30m-like: B 32, n 27, seq_len 70)": dict(n_agents=27, obs_shape=348, n_actions=36, state_shape=1170, episode_limit=70),
}
# launches of one train, counted from the call sequence of xt_qmix_step / xt_qmix_apply: agents' forward 9 (6 Dense, 1 recurrent,
# 2 dense_1), hypernets 14, head 3, hypernets' backward 17, agent's backward 16 (1 recurrent), optimiser 2
LAUNCHES = 9 + 14 + 3 + 17 + 16 + 2


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    out = np.asarray(out)
    return dict(median_ms=float(np.median(out)), min_ms=float(out.min()), max_ms=float(out.max()), reps=int(reps))


def eager_step(spec, case, params, slots, lr, clip, gamma=0.99):
    """the same train in eager PyTorch (float32, autograd), centred RMSProp with per-tensor clipping included"""
    p = {k: v.requires_grad_(k.startswith("eval")) for k, v in params.items()}
    b = case["obs"].shape[0]
    h0 = torch.zeros(b * spec.n, spec.H, device="cuda")
    qe, _ = Q.agent_ref(p, "eval_agent", case["obs"], case["lens"], h0)
    qt, _ = Q.agent_ref(p, "target_agent", case["obs"], case["lens"], h0)
    he = Q.hyp_rows(p, "eval_mixer", case["cur"].reshape(b * spec.T, -1))
    ht = Q.hyp_rows(p, "target_mixer", case["nxt"].reshape(b * spec.T, -1))
    loss = Q.head_ref(qe, qt, case["avail"], case["actions"], he, ht, case["rewards"], case["terminated"], case["mask"], gamma,
                      spec.double_q, spec.E)[0]
    ev = [k for k in p if k.startswith("eval")]
    grads = torch.autograd.grad(loss, [p[k] for k in ev])
    with torch.no_grad():
        for k, g in zip(ev, grads):
            g = g * clip / torch.clamp(g.norm(), min=clip)
            mg, ms = slots[k]
            ms += (g * g - ms) * 0.05
            mg += (g - mg) * 0.05
            p[k] -= lr * g / torch.sqrt(ms - mg * mg + 1.5e-7)
    return loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--eager-reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L.require_gpu()
    lib = L.load()
    report = dict(launches_per_train=LAUNCHES)
    for name, dims in SHAPES.items():
        spec = QMixSpec(dict(dims, rnn_hidden_dim=64, mixing_embed_dim=32, hypernet_embed=64, batch_size=32))
        net = HipQmix(spec, seed=0)
        case = Q.make_case(spec, 32, 7)
        net.grad_step(*Q.train_args(case))              # stages the batch on the device (net._keep)
        ptrs = [L.ptr(x) for x in net._keep]

        def hip_train():
            L.check(lib.xt_qmix_step(net.handle, *ptrs, 32, ctypes.byref(net.cfg), L.ptr(net.loss_dev), L.stream_ptr()), "step")
            L.check(lib.xt_qmix_apply(net.handle, ctypes.byref(net.cfg), L.stream_ptr()), "apply")

        row = dict(hip_train=timed(hip_train, args.reps))
        # the two persistent kernels alone, on random inputs of the same shape
        t1, s, h = spec.T + 1, 32 * spec.n, spec.H
        g = Q.gru_case(s, t1, h, False)
        d = {k: torch.from_numpy(v).cuda() for k, v in g.items()}
        saved, out, dg3 = (torch.empty(t1, s, k * h, device="cuda") for k in (4, 1, 3))
        fwd = lambda: L.check(lib.xt_qmix_gru_fwd(L.ptr(d["wg"]), L.ptr(d["wc"]), L.ptr(d["xg"]), None, None, t1, s, h, L.ptr(saved),    # noqa: E731
                                                  L.ptr(out), None, L.stream_ptr()), "gru_fwd")
        bwd = lambda: L.check(lib.xt_qmix_gru_bwd(L.ptr(d["wg"]), L.ptr(d["wc"]), L.ptr(saved), None, L.ptr(d["dout"]), None, None, t1,  # noqa: E731
                                                  s, h, L.ptr(dg3), None, L.stream_ptr()), "gru_bwd")
        for key, fn in (("gru_fwd", fwd), ("gru_bwd", bwd)):
            row[key] = timed(fn, args.reps)
            row[key]["per_step_us"] = 1e3 * row[key]["median_ms"] / t1
        # eager PyTorch, same device
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
        ecase = dict(obs=dev(case["obs"]), lens=dev(np.asarray(case["lens"]).astype(np.int64)), avail=dev(case["avail"]),
                     actions=dev(case["actions"][..., 0].astype(np.int64)), cur=dev(case["cur"]), nxt=dev(case["nxt"]),
                     rewards=dev(case["rewards"][..., 0]), terminated=dev(case["terminated"][..., 0]), mask=dev(case["mask"][..., 0]))
        eparams = {k: dev(v) for k, v in Q.make_params(spec, 1).items()}
        slots = {k: (torch.zeros_like(v), torch.ones_like(v)) for k, v in eparams.items() if k.startswith("eval")}
        row["eager_train"] = timed(lambda: eager_step(spec, ecase, eparams, slots, 0.0005, 10.0), args.eager_reps, warm=2)
        report[name] = row
        print(name, json.dumps(row))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
