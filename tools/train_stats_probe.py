"""The cost of ``TRAIN_STATS``: one PPO update at the headline shape with the key off against on, alternating in one process.

    python tools/train_stats_probe.py [--updates 30] [--warmup 3] [--out profiles/train_stats.md]

Two ``PpoCnn`` models (84x84x4 uint8, A = 4, hidden [256]) are built from the same SEED, one without the key and one with
it, and fed the same rollout of n = 4096 rows (BATCH_SIZE 320, NUM_SGD_ITER 4: 52 SGD steps per update, one replayed
hipGraph).  Both are warmed up (the first update captures the graph) and then timed alternately with a host clock around
``train``, which returns once the loss -- and with the key on the 128 bytes of sums in front of it -- has reached the host.
The second table holds the error of the sums of one gradient-only step against float64 on the nets of
tests/test_gpu_train_stats.py (its case 1).  Writes a markdown file; needs a GPU.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

N, BATCH, EPOCHS = 4096, 320, 4


def build(on):
    from xingtian_amd.model import model_builder
    cfg = dict(BATCH_SIZE=BATCH, NUM_SGD_ITER=EPOCHS, hidden_sizes=[256], SEED=7, DEVICE="gpu", USE_HIP_GRAPH=True)
    if on:
        cfg["TRAIN_STATS"] = True
    return model_builder(dict(model_name="PpoCnn", state_dim=[84, 84, 4], action_dim=4, input_dtype="uint8",
                              model_config=cfg))


def spread(ms):
    q = np.percentile(ms, [0, 25, 50, 75, 100])
    return dict(min=q[0], q1=q[1], median=q[2], q3=q[3], max=q[4])


def timed(model, state, label, perms):
    t0 = time.perf_counter()
    model.train(state, label, perms=perms)      # (returns the loss as a host number: a host clock is a device-complete time)
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_stats.md"))
    args = ap.parse_args()
    import torch
    from xingtian_amd import lib
    lib.require_gpu()
    rng = np.random.default_rng(3)
    obs = rng.integers(0, 256, (N, 84, 84, 4)).astype(np.uint8)
    action = rng.integers(0, 4, N).astype(np.int32)
    logp = (-np.abs(rng.standard_normal((N, 1))) - 0.5).astype(np.float32)
    adv = rng.standard_normal((N, 1))
    old_v = rng.standard_normal((N, 1)).astype(np.float32)
    target_v = old_v.astype(np.float64) + rng.standard_normal((N, 1))
    state, label = [obs], [action, logp, adv, old_v, target_v]
    perms = np.stack([rng.permutation(N) for _ in range(EPOCHS)]).astype(np.int32)
    models = {"off": build(False), "on": build(True)}
    for _ in range(args.warmup):
        for m in models.values():
            m.train(state, label, perms=perms)
    ms = {"off": [], "on": []}
    for i in range(args.updates):
        for k in (("off", "on") if i % 2 == 0 else ("on", "off")):
            ms[k].append(timed(models[k], state, label, perms))
    d = models["on"].train_stats()
    assert models["off"].train_stats() is None and d["steps"] == 52.0 and d["rows"] == float(N * EPOCHS)
    s = {k: spread(v) for k, v in ms.items()}
    cell = lambda x: "{median:.3f} ({q1:.3f}-{q3:.3f}, {min:.3f}-{max:.3f})".format(**x)
    steps = EPOCHS * ((N + BATCH - 1) // BATCH)
    delta = s["on"]["median"] - s["off"]["median"]
    if s["off"]["q3"] < s["on"]["q1"]:
        word = "slower beyond the spread (the key-off third quartile is below its first)"
    elif s["on"]["q3"] < s["off"]["q1"]:
        word = "faster beyond the spread"
    else:
        word = "not apart from the key-off update beyond the spread"
    lines = ["# PPO update: `TRAIN_STATS` off against on", "",
             "`tools/train_stats_probe.py`, {} on {}; kernel-source digest `{}`.  PpoCnn 84x84x4 uint8, A = 4, hidden [256], "
             "n = {}, BATCH_SIZE {}, NUM_SGD_ITER {} ({} SGD steps per update, one replayed hipGraph).  Key off and key on "
             "alternate in one process after {} warm-up updates of each; {} timed updates of each, host clock around "
             "`train(state, label)` (upload of the rollout, the update, the read-back of the loss; with the key on also the "
             "128 bytes of sums in front of the loss).  The key-off path is the code of the parent commit, unchanged in this "
             "tree.".format("torch " + torch.__version__, torch.cuda.get_device_name(0), lib.built_sources_sha(), N, BATCH,
                            EPOCHS, steps, args.warmup, args.updates), "",
             "| | ms per update (median, q1-q3, min-max) |", "|---|---|",
             "| key off | {} |".format(cell(s["off"])), "| key on | {} |".format(cell(s["on"])), "",
             "With the key on the update is {}: {:+.3f} ms per update at the medians, {:+.2f} us per SGD step ({:+.2f} %).".format(
                 word, delta, delta * 1e3 / steps, 100.0 * delta / s["off"]["median"]), "",
             "The statistics of the last timed update: " + ", ".join("`{}` {:.6g}".format(k, v) for k, v in d.items()) + "."]
    print("\n".join(lines[6:]), flush=True)
    del models
    import test_gpu_train_stats as T
    notes = ["", "## Error of the sums of one step against float64", "",
             "The nets and the rollout of tests/test_gpu_train_stats.py (case 1: one gradient-only step on 40 and on 16 rows; "
             "reference = numpy float64 on the fp32 logits / mean / value of `forward`).  Per quantity the larger of the two "
             "errors of its per-row (per-step) mean and the test's bar `max(1e-4 |ref|, 1e-6)`; the step, row and flag counts "
             "are exact.", "", "| net | head path | " + " | ".join(("SURR", "ENT", "VF", "KL", "TV", "TV_SQ", "ERR", "ERR_SQ")) + " |",
             "|---|---|" + "---|" * 8]
    for kind in sorted(T.NETS):
        path, worst = T.one_step_errors(kind)
        notes.append("| {} | {:#x} | ".format(kind, path) + " | ".join(
            "{:.1e} / {:.1e}".format(*worst[k]) for k in ("SURR", "ENT", "VF", "KL", "TV", "TV_SQ", "ERR", "ERR_SQ")) + " |")
        print(notes[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines + notes) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
