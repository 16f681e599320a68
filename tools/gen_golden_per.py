"""Golden vectors of the reference's prioritised replay, produced by EXECUTING the reference.

``xt/algorithm/prioritized_replay_buffer_muzero.py::PrioritizedReplayBuffer`` and ``xt/algorithm/segment_tree.py`` are
loaded with importlib under stub ``xt`` / ``xt.algorithm`` packages (the pattern of ``oracle/gen_golden_alg.py``; the
two files import nothing else of the reference).  Each case runs a script of messages (``add`` per transition, priority
``None``) and ``update_priorities`` batches on one buffer, then one ``sample(B, beta)`` under ``random.seed(7)``.

Two case tables, one file each: ``CASES`` -> tests/golden/per_cases.npz (batches of at most 256 rows on rings of at most
1000), ``WIDE_CASES`` -> tests/golden/per_cases_wide.npz (update batches of 65 to 1024 rows: every workgroup size the
update kernel launches between 64 and 1024 threads that these give, duplicates more than 255 rows apart).

Recorded per case ``<c>`` (data only; nothing at test time reads the reference):
  <c>_cfg       float64 [5]: BUFFER_SIZE, N (stored transitions at the end), B, alpha, beta
  <c>_msg_lens  int64: the message lengths
  <c>_script    int64: k >= 0 -> message k is added, -1 -> the next update batch is applied
  <c>_upd_idx / <c>_upd_prio / <c>_upd_splits: all update batches concatenated, and where each one ends
  <c>_leaves    float64 [cap2]: the sum tree's leaves;  <c>_sum / <c>_min: both full trees [2 * cap2]
  <c>_max_prio  the final _max_priority
  <c>_u         float64 [B]: the draws ``sample`` consumed (edge cases: the first three and the last replaced by 0.0 and
                1 - 2**-53)
  <c>_p_total, <c>_idx [B], <c>_w [B]: what ``sample`` computed

Usage:  python tools/gen_golden_per.py [--table base|wide] [reference root]     (no --table: both files are rewritten)
"""
import importlib.util
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")
SEED = 7

# name: (BUFFER_SIZE, message lengths, B, alpha, beta, edge draws)
CASES = {
    "c5": (5, (3, 9), 32, 0.6, 0.4, False),                  # one message longer than the capacity, wrapping twice
    "c37": (37, (20, 30), 33, 0.6, 0.4, False),              # wraps
    "c707": (1000, (300, 407), 256, 0.6, 0.4, False),        # N < capacity
    "c1000": (1000, (600, 700), 1, 0.6, 0.4, False),         # wraps, one sample
    "c64": (64, (64, 10), 32, 0.6, 0.4, False),              # capacity a power of two
    "c37_alpha1": (37, (20, 30), 33, 1.0, 0.4, False),
    "c37_beta1": (37, (20, 30), 33, 0.6, 1.0, False),
    "c64_edge": (64, (64, 10), 32, 0.6, 0.4, True),
}

WIDE_CASES = {
    "w1000_b1024": (1000, (700, 650), 1024, 0.6, 0.4, False),  # batches of 700 / 952 / 1024 rows, duplicates in every one
    "w330_b320": (330, (200, 250), 320, 0.6, 0.4, True),       # 200 / 320 / 30 rows; slot N - 1 drawn by 1 - 2**-53
    "w140_b129": (140, (90, 40), 129, 1.0, 1.0, False),        # 90 / 129 / 3 rows; N < capacity
    "w100_b65": (100, (100, 30), 65, 0.6, 0.4, False),         # 65 / 35 / 40 rows
}
TABLES = {"base": ("per_cases.npz", CASES), "wide": ("per_cases_wide.npz", WIDE_CASES)}


def load_reference(ref):
    for name in ("xt", "xt.algorithm"):
        if name not in sys.modules:
            pkg = type(sys)(name)
            pkg.__path__ = []
            sys.modules[name] = pkg
    mods = []
    for name, path in (("xt.algorithm.segment_tree", "xt/algorithm/segment_tree.py"),
                       ("xt.algorithm.prioritized_replay_buffer_muzero", "xt/algorithm/prioritized_replay_buffer_muzero.py")):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref, path))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods[1].PrioritizedReplayBuffer


def run_case(cls, name, case, out):
    capacity, msg_lens, b, alpha, beta, edge = case
    rng = np.random.default_rng(sum(map(ord, name)))
    buf = cls(capacity, alpha)
    script, idx_all, prio_all, splits, tag = [], [], [], [], 0

    def updates(total):
        done = 0
        while done < total:
            k = min(b, total - done)
            idx = rng.integers(0, len(buf), k)
            prio = rng.uniform(1e-3, 5.0, k)
            buf.update_priorities([int(i) for i in idx], [float(p) for p in prio])
            idx_all.extend(idx.tolist())
            prio_all.extend(prio.tolist())
            splits.append(len(idx_all))
            script.append(-1)
            done += k

    for k, n in enumerate(msg_lens):
        for _ in range(n):
            buf.add(tag)
            tag += 1
        script.append(k)
        if k == 0:
            updates(len(buf))                # raises _max_priority before the later messages are added
    n_stored = len(buf)
    updates(3 * n_stored)
    cap2 = buf._it_sum._capacity
    random.seed(SEED)
    u = [random.random() for _ in range(b)]
    if edge:
        u[0], u[-1] = 0.0, 1.0 - 2.0 ** -53
        u[1], u[2] = 1.0 - 2.0 ** -53, 0.0
    draws = iter(u)
    real = random.random
    random.random = lambda: next(draws)      # (the reference draws from the global module)
    try:
        _, weights, idxes = buf.sample(b, beta)
    finally:
        random.random = real
    assert next(draws, None) is None and max(idxes) < n_stored
    pre = name + "_"
    out[pre + "cfg"] = np.array([capacity, n_stored, b, alpha, beta], np.float64)
    out[pre + "msg_lens"] = np.array(msg_lens, np.int64)
    out[pre + "script"] = np.array(script, np.int64)
    out[pre + "upd_idx"] = np.array(idx_all, np.int64)
    out[pre + "upd_prio"] = np.array(prio_all, np.float64)
    out[pre + "upd_splits"] = np.array(splits, np.int64)
    out[pre + "leaves"] = np.array(buf._it_sum._value[cap2:], np.float64)
    out[pre + "sum"] = np.array(buf._it_sum._value, np.float64)
    out[pre + "min"] = np.array(buf._it_min._value, np.float64)
    out[pre + "max_prio"] = np.float64(buf._max_priority)
    out[pre + "u"] = np.array(u, np.float64)
    out[pre + "p_total"] = np.float64(buf._it_sum.sum(0, n_stored - 1))
    out[pre + "idx"] = np.array(idxes, np.int64)
    out[pre + "w"] = np.array(weights, np.float64)
    print("{}: capacity {} cap2 {} N {} B {} | {} update batches, max_priority {:.6f}, {} distinct of {} samples, "
          "largest index {}".format(name, capacity, cap2, n_stored, b, len(splits), buf._max_priority, len(set(idxes)), b,
                                    max(idxes)))


def main():
    argv, tables = sys.argv[1:], sorted(TABLES)
    if argv[:1] == ["--table"]:
        tables, argv = [argv[1]], argv[2:]
    if argv:
        ref = argv[0]
    else:
        from oracle.gen_golden_alg import REF as ref
    cls = load_reference(ref)
    for table in tables:
        fname, cases = TABLES[table]
        out = {"names": np.array(sorted(cases))}
        for name in sorted(cases):
            run_case(cls, name, cases[name], out)
        path = os.path.join(GOLDEN, fname)
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
