"""``predict`` with ``PREDICT_ON_DEVICE`` off against on, alternating in one process.

    python tools/act_probe.py [--calls 200] [--warmup 3] [--out profiles/act_on_device.md]

Per shape two models are built from the same SEED, one with the key off (the host path: logits and value copied back,
sampling and log-probability in numpy) and one with it on (``xt_net_act``: one head launch, one packed copy).  Both are
warmed up and then timed alternately with a host clock around ``predict(obs)``; ``obs`` is a host array, as an explorer
hands it over, and either path ends in a synchronising copy to the host.  The second table holds the error of the
log-probability against float64 on the cases of tests/test_gpu_act.py (G3), device path and host expressions side by side.
Writes a markdown file; needs a GPU.
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

PPO_CNN = dict(model_name="PpoCnn", state_dim=[84, 84, 4], action_dim=4, input_dtype="uint8")
IMPALA = dict(model_name="ImpalaCnnOpt", state_dim=[42, 42, 4], action_dim=6, input_dtype="uint8", state_mean=128.0,
              state_std=128.0)
SHAPES = [("PpoCnn [84,84,4] uint8, A=4, B=%d" % b, PPO_CNN, {}, (b, 84, 84, 4), np.uint8) for b in (1, 32, 250, 1024)]
SHAPES += [("ImpalaCnnOpt [42,42,4] uint8, A=6, B=250", IMPALA, {}, (250, 42, 42, 4), np.uint8),
           ("PpoMlp [4], A=2, B=10", dict(model_name="PpoMlp", state_dim=[4], action_dim=2), {}, (10, 4), np.float32)]


def build(info, cfg, on):
    from xingtian_amd.model import model_builder
    return model_builder(dict(info, model_config=dict(cfg, SEED=7, DEVICE="gpu", PREDICT_ON_DEVICE=on)))


def spread(ms):
    q = np.percentile(ms, [0, 25, 50, 75, 100])
    return dict(min=q[0], q1=q[1], median=q[2], q3=q[3], max=q[4])


def timed(model, obs):
    t0 = time.perf_counter()
    model.predict(obs)                         # (returns host arrays: a host clock is a device-complete time)
    return (time.perf_counter() - t0) * 1e3


def logp_errors():
    """(case, device error, host-expression error, bound) of G3, on the test's own cases"""
    import act_helpers as H
    import test_gpu_act as T
    rows = []
    for gauss, shapes in ((False, T.CAT_SHAPES), (True, T.GAUSS_SHAPES)):
        for shape in shapes:
            c = T.kernel_case(shape, gauss)
            out = c["out"]
            if gauss:
                ref = H.gauss_logp_ref(out["logits"], c["log_std"], out["action"])
                host = H.gauss_logp_host(out["logits"], c["log_std"], out["action"])
            else:
                ref = H.cat_logp_ref(out["logits"], out["action"])
                host = H.cat_logp_host(out["logits"], out["action"])
            e_dev = np.abs(out["logp"].reshape(-1) - ref.reshape(-1)).max()
            e_host = np.abs(host.reshape(-1) - ref.reshape(-1)).max()
            rows.append(("%s (B, F, A) = %s" % ("DiagGaussian" if gauss else "Categorical", shape), e_dev, e_host,
                         H.logp_bound(e_host, ref)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "act_on_device.md"))
    args = ap.parse_args()
    import torch
    from xingtian_amd import lib
    lib.require_gpu()
    lines = ["# predict: host sampling against device sampling (`PREDICT_ON_DEVICE`)", "",
             "`tools/act_probe.py`, {} on {}; kernel-source digest `{}`.  Key off and key on alternate in one process after {} "
             "warm-up calls of each; {} timed calls of each, host clock around `predict(obs)` with `obs` a host array (either "
             "path ends in a synchronising copy to the host).  The key-off path is the code of the parent commit, unchanged "
             "in this tree.".format("torch " + torch.__version__, torch.cuda.get_device_name(0), lib.built_sources_sha(),
                                    args.warmup, args.calls), "",
             "| shape | key off ms (median, q1-q3, min-max) | key on ms (median, q1-q3, min-max) | off / on |",
             "|---|---|---|---|"]
    verdicts = []
    for name, info, cfg, shape, dtype in SHAPES:
        models = {"off": build(info, cfg, False), "on": build(info, cfg, True)}
        assert models["off"]._act is None and models["on"]._act is not None
        rng = np.random.default_rng(1)
        draw = (lambda: rng.integers(0, 256, shape).astype(dtype)) if dtype == np.uint8 else \
            (lambda: rng.standard_normal(shape).astype(dtype))
        pool = [draw() for _ in range(4)]
        for w in range(args.warmup):
            for m in models.values():
                m.predict(pool[w % len(pool)])
        ms = {"off": [], "on": []}
        for i in range(args.calls):
            obs = pool[i % len(pool)]
            for k in (("off", "on") if i % 2 == 0 else ("on", "off")):
                ms[k].append(timed(models[k], obs))
        s = {k: spread(v) for k, v in ms.items()}
        cell = lambda d: "{median:.3f} ({q1:.3f}-{q3:.3f}, {min:.3f}-{max:.3f})".format(**d)
        lines.append("| {} | {} | {} | {:.2f} |".format(name, cell(s["off"]), cell(s["on"]),
                                                      s["off"]["median"] / s["on"]["median"]))
        if s["on"]["q3"] < s["off"]["q1"]:
            word = "faster beyond the spread (its third quartile is below the host path's first)"
        elif s["off"]["q3"] < s["on"]["q1"]:
            word = "SLOWER beyond the spread (the host path's third quartile is below its first)"
        else:
            word = "not apart from the host path beyond the spread"
        verdicts.append("- {}: the device path is {} ({:.3f} against {:.3f} ms median).".format(
            name, word, s["on"]["median"], s["off"]["median"]))
        print(lines[-1])
        print(verdicts[-1], flush=True)
        del models
    notes = ["", "## Error of the log-probability against float64", "",
             "The cases of tests/test_gpu_act.py (random features and head weights, injected noise): `max |logp - ref|` of the "
             "device path and of the host path's numpy expressions on the same logits and actions, and the test's bound "
             "`4 e_host + 4 * 2^-24 * (1 + max |ref|)`.", "", "| case | device | host expressions | bound |", "|---|---|---|---|"]
    for row in logp_errors():
        notes.append("| {} | {:.3g} | {:.3g} | {:.3g} |".format(*row))
        print(notes[-1])
    text = "\n".join(lines + [""] + verdicts + notes) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
