"""The cost of ``TRAIN_STATS`` on the IMPALA path, and the error of its sums: key off against on, alternating in one process.

    python tools/impala_stats_probe.py [--pairs 7] [--reps 10] [--resources FILE] [--out profiles/impala_stats.md]

For breakout_impala (84x84x4, A = 4, T = 128, one 128-frame train) and pong_impala_speedup (42x42x4, A = 6, T = 50, one
1000-frame train) two nets are built from the same seed, one with ``xt_net_set_impala_stats`` and one without, and run as
``bench.py`` runs them: ``trains`` one-chunk trains enqueued by ONE ``xt_net_impala_train`` call (one replayed hipGraph),
``--reps`` such calls per measurement, a device synchronisation, ``us_per_train`` = time / (reps x trains).  Both are warmed
up, then measured in ``--pairs`` pairs, off first in even pairs and on first in odd ones.  The second part runs the kernel
cases of tests/test_gpu_impala_stats.py and reports, per path, the figure nearest its bar.  ``--resources``: a markdown
file with the compiler's register / scratch / LDS report (made where hipcc is), appended as it is.  Needs a GPU.
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

WORKLOADS = {   # bench.py IMPALA: shape, frames per train, trains per call
    "breakout_impala": dict(dim=84, a_dim=4, t_len=128, frames=128, mean=0.0, std=255.0, lr=5e-4, trains=64),
    "pong_impala_speedup": dict(dim=42, a_dim=6, t_len=50, frames=1000, mean=128.0, std=128.0, lr=1e-3, trains=16),
}


def measure(key, pairs, reps, warmup=3):
    import torch
    from xingtian_amd.model import netspec
    from xingtian_amd.model.hip_net import HipActorCritic
    w = WORKLOADS[key]
    f, trains = w["frames"], w["trains"]
    n = f * trains
    rng = np.random.default_rng(7)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    bufs = [d(rng.integers(0, 256, (n, w["dim"], w["dim"], 4)).astype(np.uint8)),
            d(rng.standard_normal((n, w["a_dim"])).astype(np.float32)), d(rng.integers(0, w["a_dim"], n).astype(np.int32)),
            d((rng.random(n) < 0.02).astype(np.uint8)), d(rng.choice([-1.0, 0.0, 1.0], n).astype(np.float32))]
    nets, cfgs = {}, {}
    for name in ("off", "on"):
        net = HipActorCritic(netspec.impala_cnn_opt((w["dim"], w["dim"], 4), w["a_dim"], w["mean"], w["std"], "uint8"),
                             max_batch=f, seed=0)
        if name == "on":
            net.set_impala_stats(True)
        nets[name], cfgs[name] = net, net.make_impala_cfg(w["lr"], 40.0, w["t_len"])

    def timed(name, count):
        net = nets[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            net.impala_train(cfgs[name], bufs[0], f, *bufs[1:], use_graph=True)
        torch.cuda.synchronize()
        return 1e6 * (time.perf_counter() - t0) / (count * trains)

    for name in nets:
        timed(name, warmup)
    rows = []
    for i in range(pairs):
        order = ("off", "on") if i % 2 == 0 else ("on", "off")
        got = {name: timed(name, reps) for name in order}
        rows.append((got["off"], got["on"]))
    from xingtian_amd.ops import impala_stats_from_sums
    s = impala_stats_from_sums(nets["on"].fetch_impala_stats())
    assert s["chunks"] == float(trains) and s["transitions"] == float(trains * (f // w["t_len"]) * (w["t_len"] - 1))
    assert torch.isfinite(nets["on"].params).all() and torch.equal(nets["on"].params, nets["off"].params)
    return np.array(rows), s


def kernel_errors():
    import impala_stats_helpers as H
    import test_gpu_impala_stats as T
    from xingtian_amd import lib as L
    out = []
    for tag, cases, run in (("fused, AM = 8", H.FUSED8, T.run_fused), ("fused, AM = 32", H.FUSED32, T.run_fused),
                            ("unfused", H.UNFUSED, T.run_unfused)):
        worst = (0.0, None, None)
        for case in cases:
            plain, _ = run(L, case, False)
            stat, _ = run(L, case, True)
            w = T.check_kernel(tag, case, plain, stat)
            if w[0] >= worst[0]:
                worst = (w[0], case, w[1])
        out.append((tag, len(cases)) + worst)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--resources", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "impala_stats.md"))
    args = ap.parse_args()
    assert args.pairs >= 5, "at least five pairs"
    import torch
    from xingtian_amd import lib
    lib.require_gpu()
    lines = ["# IMPALA trains: `TRAIN_STATS` off against on", "",
             "`tools/impala_stats_probe.py`, torch {} on {}; kernel-source digest `{}`.  Per workload two nets from one seed, "
             "one with `xt_net_set_impala_stats`; as in `bench.py`, `trains` one-chunk trains are enqueued by one "
             "`xt_net_impala_train` call (one replayed hipGraph), {} calls per measurement, `us_per_train` = time / (calls x "
             "trains).  {} pairs, off first in even pairs, on first in odd ones.  The key-off path is the code of the parent "
             "commit.".format(torch.__version__, torch.cuda.get_device_name(0), lib.built_sources_sha(), args.reps, args.pairs),
             ""]
    for key in WORKLOADS:
        rows, s = measure(key, args.pairs, args.reps)
        off, on = rows[:, 0], rows[:, 1]
        lines += ["## {} ({} frames per train, {} trains per call)".format(key, WORKLOADS[key]["frames"],
                                                                          WORKLOADS[key]["trains"]), "",
                  "| pair | off us_per_train | on us_per_train | on - off |", "|---|---|---|---|"]
        lines += ["| {} | {:.2f} | {:.2f} | {:+.2f} |".format(i, a, b, b - a) for i, (a, b) in enumerate(rows)]
        lines += ["", "Median off {:.2f} (min {:.2f}, max {:.2f}), median on {:.2f} (min {:.2f}, max {:.2f}): {:+.2f} us per "
                  "train at the medians ({:+.2f} %); the pair differences run from {:+.2f} to {:+.2f} us.".format(
                      np.median(off), off.min(), off.max(), np.median(on), on.min(), on.max(), np.median(on) - np.median(off),
                      100.0 * (np.median(on) - np.median(off)) / np.median(off), (on - off).min(), (on - off).max()), "",
                  "The statistics of the last call: " + ", ".join("`{}` {:.6g}".format(k, v) for k, v in s.items()) + ".", ""]
        print("\n".join(lines[-(args.pairs + 8):]), flush=True)
    lines += ["## Error of the trajectory rows against float64", "",
              "The kernel cases of tests/test_gpu_impala_stats.py (logits given, the recipe of tests/impala_stats_helpers.py): "
              "per path the figure nearest its bar over all cases, trajectories and columns.  Bars: `max(1e-4 |ref|, 1e-6)`; "
              "`1e-4 sum|term| + 1e-6` for the sums that can cancel (columns 0, 3, 6).  The counts of rho > 1 and of "
              "transitions are exact, and the six existing outputs equal those of the existing entries bit for bit.", "",
              "| path | cases | nearest its bar: err / bar | case (n_traj, T, A) | column, trajectory, got, ref, err, bar |",
              "|---|---|---|---|---|"]
    errs = kernel_errors()
    for tag, ncase, ratio, case, detail in errs:
        lines.append("| {} | {} | {:.3f} | {} | {} |".format(tag, ncase, ratio, case,
                                                            ", ".join("{:.6g}".format(x) for x in detail)))
    top = max(errs, key=lambda e: e[2])
    lines += ["", "The figure nearest its bar of all: {} at {} of its bar (case {}).".format(top[0], "%.3f" % top[2], top[3]), ""]
    if args.resources and os.path.exists(args.resources):
        lines += open(args.resources).read().rstrip("\n").split("\n")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
