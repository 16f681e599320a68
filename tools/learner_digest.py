"""Digests of the bits the MuZero, QMIX and SCC learners produce on small seeded cases: the check of a change that must not
move a bit (profiles/dense_share_parity.md).  Every case runs one step, then two further trains with the optimiser (QMIX / SCC:
a target sync before the last), and prints the first 16 hex digits of the sha256 of
  loss   the three trains' loss words
  grad   the flat gradient after the first step
  state  the flat parameters (QMIX / SCC: and the target set) and the optimiser slots at the end
The cases cover one and several weight-gradient slabs (128 rows for MuZero, 512 for QMIX / SCC), row counts that are no multiple
of 4, ragged lengths, double-Q on and off, both channel merges, two agent groups and both alternatives of the credits.
It needs the tests' helpers only: copy it next to a checkout of another commit to compare the two.

    python tools/learner_digest.py [--out digests.json]
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import muzero_helpers as MH                                 # noqa: E402
from tests import qmix_helpers as Q                                    # noqa: E402
from tests import scc_helpers as S                                     # noqa: E402
from xingtian_amd import lib as L                                      # noqa: E402

PONG = dict(value_range=(-21, 21), reward_range=(-2, 2))            # supports 7 / 3
DEFAULT = dict(value_range=(0, 60000), reward_range=(-300, 300))    # supports 305 / 26


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t).tobytes())
    return h.hexdigest()


def three_trains(net, step, state):
    """step() -> the loss tensor; -> the three digests"""
    losses, grad = [], None
    for i in range(3):
        if i == 2 and hasattr(net, "sync_target"):
            net.sync_target()
        losses.append(step().cpu().numpy().copy())
        if i == 0:
            grad = sha(net.grads)
        net.apply()
    return dict(loss=sha(*losses), grad=grad, state=sha(*state(net)))


def muzero(b, unroll, ranges, seed):
    from xingtian_amd.model.muzero.muzero_model import HipMuzero, mlp_spec
    spec = mlp_spec((4,), 2, 64, 4, unroll, **ranges)
    net = HipMuzero(spec, max_batch=b, seed=seed)
    net.set_weights(MH.seeded_weights(spec, seed))
    batch = MH.make_batch(spec, b, seed + 1)
    return three_trains(net, lambda: net.grad_step(*batch), lambda n: (n.params, n.adam_m, n.adam_v, n.adam_state))


def qmix(b, n, t, h, double_q, seed):
    from xingtian_amd.model.qmix.qmix_model import HipQmix
    spec = Q.make_spec(n=n, t=t, h=h, batch=b, double_q=double_q)
    net = HipQmix(spec, seed=0, lr=0.01, clip=0.5)
    for which in ("eval", "target"):
        net.set_train_weights(Q.make_params(spec, seed), which)
    args = Q.train_args(Q.make_case(spec, b, 100 + seed, 4.0))
    return three_trains(net, lambda: net.grad_step(*args), lambda n: (n.params, n.target, n.mg, n.ms, n.state))


def scc(b, n, groups, merge, t, h, u, seed):
    from xingtian_amd.model.scc.scc_model import HipScc
    spec = S.make_spec(n=n, groups=groups, merge=merge, u=u, h=h, t=t, batch=b)
    net = HipScc(spec, seed=0, c_lr=0.01, a_lr=0.01, mixer_clip=0.3, actor_clip=0.02)
    for which in ("eval", "target"):
        net.set_train_weights(S.make_params(spec, seed), which)
    a = S.train_args(S.make_case(spec, b, 100 + seed))
    return three_trains(net, lambda: net.grad_step(a[0], a[1], a[2], a[4], *a[7:]),
                        lambda n: (n.params, n.target, n.slot1, n.slot2, n.state))


CASES = [
    # MuZero: stacked rows (U + 1) B and U B against the slab height 128
    ("muzero B 5 U 3 supports 7/3 (rows 20 / 15: no multiple of 4, one slab)", lambda: muzero(5, 3, PONG, 3)),
    ("muzero B 50 U 3 supports 305/26 (rows 200 / 150: two slabs)", lambda: muzero(50, 3, DEFAULT, 4)),
    # QMIX: M = (T + 1) B n stacked rows against the slab height 512; ragged lengths in both
    ("qmix B 3 n 2 T 5 H 32 double_q (M 36: one slab)", lambda: qmix(3, 2, 5, 32, True, 1)),
    ("qmix B 8 n 3 T 24 H 64 plain (M 600: two slabs)", lambda: qmix(8, 3, 24, 64, False, 2)),
    # SCC: n = 2 takes the alt_zero branch of the credits, n = 3 the other
    ("scc B 3 n 2 T 4 concat H 32 U 32 (M 30)", lambda: scc(3, 2, None, "concat", 4, 32, 32, 1)),
    ("scc B 2 n 3 groups (1, 2) T 4 add H 64 U 32 (M 30)", lambda: scc(2, 3, (1, 2), "add", 4, 64, 32, 2)),
    ("scc B 8 n 3 groups (1, 2) T 24 concat H 32 U 64 (M 600: two slabs)", lambda: scc(8, 3, (1, 2), "concat", 24, 32, 64, 3)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    L.require_gpu()
    report = {}
    for name, run in CASES:
        report[name] = run()
        print("{}: {}".format(name, " ".join("{} {}".format(k, v[:16]) for k, v in report[name].items())), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
