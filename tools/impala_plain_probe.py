"""Non-opt ``IMPALA.train``: host path against device path (``DEVICE_VTRACE``), alternating in one process.

    python tools/impala_plain_probe.py [--trains 20] [--warmup 3] [--out profiles/impala_device_train.md]

Two shapes: ``cartpole_impala.yaml``'s own (ImpalaMlp, [4], A = 2, episode_len 200, two fragments, BATCH_SIZE 800) and
ImpalaCnn on [84, 84, 4] uint8 frames (A = 4, T = 128, 8 fragments, BATCH_SIZE 512).  Per shape two algorithms are built
from the same SEED.  The FIRST train of each (same rollout, same shuffles) gives the one-train difference in loss
between the paths; then both are warmed up and timed alternately with a host clock around ``train()``, which ends in the
loss read-back on either path.  The rollout is handed over (``prepare_data``) outside the timed window.  Writes a
markdown table; needs a GPU.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {
    "cartpole_impala.yaml (ImpalaMlp [4], A=2, T=200, 2 fragments, BATCH_SIZE 800)":
        dict(model="ImpalaMlp", state_dim=[4], a=2, t=200, frags=2, batch=800, u8=False),
    "ImpalaCnn [84,84,4] uint8, A=4, T=128, 8 fragments, BATCH_SIZE 512":
        dict(model="ImpalaCnn", state_dim=[84, 84, 4], a=4, t=128, frags=8, batch=512, u8=True),
}


def build(shape, device_vtrace):
    from xingtian_amd.algorithm import alg_builder
    info = {"actor": {"model_name": shape["model"], "state_dim": shape["state_dim"], "action_dim": shape["a"],
                      "model_config": {"SEED": 7, "NUM_LAYERS": 1, "HIDDEN_SIZE": 128, "LR": 3e-4, "ENTROPY_LOSS": 0.01}}}
    cfg = {"instance_num": shape["frags"], "agent_num": 1, "prepare_times_per_train": shape["frags"],
           "BATCH_SIZE": shape["batch"], "episode_len": shape["t"], "GAMMA": 0.99, "DEVICE_VTRACE": device_vtrace}
    return alg_builder("IMPALA", info, cfg)


def rollout(shape, seed):
    rng = np.random.default_rng(seed)
    t, a, sd = shape["t"], shape["a"], tuple(shape["state_dim"])
    msgs = []
    for _ in range(shape["frags"]):
        beh = rng.random((t, a)) + 0.1
        msgs.append({"cur_state": (rng.integers(0, 256, (t + 1,) + sd).astype(np.uint8) if shape["u8"]
                                   else rng.uniform(-1, 1, (t + 1,) + sd).astype(np.float32)),
                     "real_action": np.eye(a, dtype=np.float32)[rng.integers(0, a, t)],
                     "reward": [float(x) for x in rng.choice([-1.0, 0.0, 1.0], t)],
                     "done": [bool(x) for x in (rng.random(t) < 0.02)],
                     "action": (beh / beh.sum(-1, keepdims=True)).astype(np.float32)})
    return msgs


def one_train(alg, msgs, shuffle_seed):
    for m in msgs:
        alg.prepare_data(m)
    np.random.seed(shuffle_seed)
    t0 = time.perf_counter()
    loss = alg.train()                       # (ends in the loss read-back: a host clock is a device-complete time)
    return (time.perf_counter() - t0) * 1e3, float(loss)


def spread(ms):
    q = np.percentile(ms, [0, 25, 50, 75, 100])
    return dict(min=q[0], q1=q[1], median=q[2], q3=q[3], max=q[4])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trains", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "impala_device_train.md"))
    args = ap.parse_args()
    import torch
    from xingtian_amd import lib
    lib.require_gpu()
    lines = ["# Non-opt IMPALA.train: host path against device path (`DEVICE_VTRACE`)", "",
             "`tools/impala_plain_probe.py`, {} on {}; kernel-source digest `{}`.  Host and device path alternate in one "
             "process after {} warm-up trains of each; {} timed trains of each, host clock around `train()` (which ends in "
             "the loss read-back on either path), the rollout handed over outside the timed window.  The host path is the "
             "code of the parent commit, unchanged in this tree.".format(
                 "torch " + torch.__version__, torch.cuda.get_device_name(0), lib.built_sources_sha(), args.warmup,
                 args.trains), "",
             "| shape | host path ms (median, q1-q3, min-max) | device path ms (median, q1-q3, min-max) | host / device |",
             "|---|---|---|---|"]
    notes = ["", "## One-train difference in loss between the paths", "",
             "Twin models (same SEED), the same rollout and the same shuffles, first train of each.  The device path takes "
             "rho from a float64 softmax of the logits and float64 logs; the host path takes it from torch's float32 "
             "softmax and float32 logs (probabilities and one-hots are float32 there).", "",
             "| shape | host loss | device loss | difference | relative |", "|---|---|---|---|---|"]
    verdicts = []
    for name, shape in SHAPES.items():
        algs = {"host": build(shape, False), "device": build(shape, True)}
        first = {k: one_train(alg, rollout(shape, 100), 1)[1] for k, alg in algs.items()}
        diff = abs(first["host"] - first["device"])
        notes.append("| {} | {:.9g} | {:.9g} | {:.3g} | {:.3g} |".format(name, first["host"], first["device"], diff,
                                                                       diff / max(abs(first["host"]), 1e-30)))
        for w in range(args.warmup):
            for k, alg in algs.items():
                one_train(alg, rollout(shape, 200 + w), 2 + w)
        ms = {"host": [], "device": []}
        for i in range(args.trains):
            msgs = rollout(shape, 300 + i)
            for k in (("host", "device") if i % 2 == 0 else ("device", "host")):
                ms[k].append(one_train(algs[k], msgs, 50 + i)[0])
        s = {k: spread(v) for k, v in ms.items()}
        cell = lambda d: "{median:.3f} ({q1:.3f}-{q3:.3f}, {min:.3f}-{max:.3f})".format(**d)
        ratio = s["host"]["median"] / s["device"]["median"]
        lines.append("| {} | {} | {} | {:.2f} |".format(name, cell(s["host"]), cell(s["device"]), ratio))
        faster = s["device"]["q3"] < s["host"]["q1"]
        verdicts.append("- {}: the device path is {} ({:.3f} against {:.3f} ms median).".format(
            name, "faster beyond the spread (its third quartile is below the host path's first)" if faster
            else "NOT faster beyond the spread", s["device"]["median"], s["host"]["median"]))
        print(lines[-1])
        print(notes[-1])
        print(verdicts[-1], flush=True)
    text = "\n".join(lines + [""] + verdicts + notes) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
