"""Time of one ``DQN.train`` at breakout_dqn's shape, beside a Keras-IMPALA step of the same trunk.

    python tools/dqn_probe.py [--windows 5] [--trains 200] [--capacity 4096] [--atoms 51] [--quantiles 51] [--noisy]
                              [--dist-dueling] [--model DqnCnn] [--out profiles/dqn_step.md]

Four things are timed at DqnCnn 84x84x4, A = 4, B = 32, each as a host clock around ``--trains`` calls that ends in a
device synchronise, after a warm-up, in ``--windows`` windows taken in turn (so that drift of the box hits all alike):

* ``DQN.train()`` as the learner loop calls it (sample, slot upload, ``xt_net_dqn_step``, ``xt_adam_keras``, the loss read
  back as a float -- one synchronisation per train), without and with ``double_dqn``;
* the same train without the read-back (``DqnModel.train_replay`` on pre-uploaded slots: what the device is given to do);
* each of the above with ``prioritized_replay`` (``xt_net_dqn_step_per``: two more launches per train, the sample in
  front and the priority update behind; the draws of ``random.random()`` go up instead of the slots);
* the uniform and the prioritised train with ``n_step: 3`` (``xt_net_dqn_step_n``: the same launches, the walk over the
  rows that follow each sampled row rides in the next-state gather), as ``DQN.train`` and enqueue only;
* with ``--atoms N`` (0: none) the distributional train (``model_config.atoms``, ``xt_net_dqn_step_dist``: the Q head is
  4 * N wide) with and without ``prioritized_replay``, ``double_dqn`` and ``n_step: 3``, as ``DQN.train`` and enqueue
  only, once on the head kernels of a marked net (wide forward, taken-action d(features)) and once, "generic", on the
  head kernels every other net runs (``set_dist_wide(False)``);
* with ``--quantiles N`` (0: none) the same arms for the quantile-regression train (``model_config.quantiles``,
  ``xt_net_dqn_step_quant``: the head is again 4 * N wide), so that ``--atoms N --quantiles N`` compares the two
  distributional heads at one width in one run;
* with ``--dist-dueling`` (and ``--atoms`` / ``--quantiles``) the arms of each head once more for the dueling network
  (``model_config.dist_dueling``: the head is 5 * N wide, ``xt_net_set_duel``), beside the non-dueling rows of the same
  run, and a third kernel arm, "generic d(features)": the wide forward with ``heads_dfeat_kernel`` behind it
  (``set_dist_wide("forward")``), which times ``heads_dfeat_duel_kernel`` against the generic kernel inside the same step;
* with ``--noisy`` the train of a noisy pair (``model_config.noisy``: ``xt_noisy_compose`` on both nets in front of the step,
  ``xt_noisy_grads`` behind it) without and with ``double_dqn``, as ``DQN.train`` and enqueue only, beside the plain rows
  of the same run, and the three added launches alone (enqueue only);
* one ``prepare_data`` of a 20-row message without and with ``prioritized_replay`` (``xt_per_add`` per written span), each
  call followed by a device synchronise;
* ``keras_impala_step`` + ``adam_keras`` on 32 rows of ``netspec.impala_cnn`` (the same trunk and heads, one network, no
  gather), enqueue only.

The ring holds ``--capacity`` transitions (a full breakout_dqn buffer is 22.6 GB; the gather reads 32 rows whatever the
capacity is).  ``--model DqnMlp`` times the same trains on the CartPole network (state 4, Dense 128) instead, with the
same A and B and without the IMPALA row.  No threshold is attached to any of these numbers.  Needs a GPU.
"""
import argparse
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

B, A_DIM, DIM = 32, 4, 84
MODEL = {"name": "DqnCnn"}                  # --model: DqnCnn (84x84x4 uint8 frames) or DqnMlp (CartPole: 4 float32)


def _states(rng, n):
    if MODEL["name"] == "DqnMlp":
        return rng.standard_normal((n, 4)).astype(np.float32)
    return rng.integers(0, 256, (n, DIM, DIM, 4), dtype=np.uint8)


def build_dqn(double, capacity, per=False, n_step=1, atoms=1, quantiles=1, noisy=False, dist_dueling=False):
    from xingtian_amd.algorithm import alg_builder
    info = {"actor": {"model_name": MODEL["name"], "type": "learner",
                      "state_dim": [4] if MODEL["name"] == "DqnMlp" else [DIM, DIM, 4], "action_dim": A_DIM,
                      "model_config": {"LR": 0.00015, "SEED": 0}}}
    if atoms > 1:
        info["actor"]["model_config"]["atoms"] = atoms
    if quantiles > 1:
        info["actor"]["model_config"]["quantiles"] = quantiles
    if noisy:
        info["actor"]["model_config"]["noisy"] = True
    if dist_dueling:
        info["actor"]["model_config"]["dist_dueling"] = True
    cfg = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 4, "BUFFER_SIZE": capacity, "BATCH_SIZE": B,
           "TARGET_UPDATE_FREQ": 1000, "double_dqn": double, "prioritized_replay": per}
    if n_step != 1:
        cfg["n_step"] = n_step
    alg = alg_builder("DQN", info, cfg)
    rng = np.random.default_rng(1)
    for _ in range(capacity // 512):
        n = 512
        alg.prepare_data({"cur_state": _states(rng, n), "next_state": _states(rng, n),
                          "action": rng.integers(0, A_DIM, n), "reward": rng.choice([-1.0, 0.0, 1.0], n),
                          "done": rng.random(n) < 0.02})
    return alg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--trains", type=int, default=200)
    ap.add_argument("--capacity", type=int, default=4096)
    ap.add_argument("--atoms", type=int, default=0)
    ap.add_argument("--quantiles", type=int, default=0)
    ap.add_argument("--noisy", action="store_true")
    ap.add_argument("--dist-dueling", action="store_true")
    ap.add_argument("--model", default="DqnCnn", choices=["DqnCnn", "DqnMlp"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    MODEL["name"] = args.model
    import torch
    from xingtian_amd.algorithm.dqn import dqn as dqn_mod
    from xingtian_amd.model import netspec
    from xingtian_amd.model.hip_net import HipActorCritic
    assert torch.cuda.is_available(), "dqn_probe needs a GPU"
    random.seed(0)
    algs = {False: build_dqn(False, args.capacity), True: build_dqn(True, args.capacity)}
    slots = {d: torch.tensor(a.buff.sample(B), dtype=torch.int32).cuda() for d, a in algs.items()}
    pers = {False: build_dqn(False, args.capacity, True), True: build_dqn(True, args.capacity, True)}
    nstep, nstep_per = build_dqn(False, args.capacity, False, 3), build_dqn(False, args.capacity, True, 3)
    nstep_slots = torch.tensor(nstep.buff.sample(B), dtype=torch.int32).cuda()
    draws = torch.tensor([random.random() for _ in range(B)], dtype=torch.float64).cuda()
    rng = np.random.default_rng(2)
    net = HipActorCritic(netspec.impala_cnn((DIM, DIM, 4), A_DIM), max_batch=B, seed=0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    obs, idx = up(rng.integers(0, 256, (B, DIM, DIM, 4), dtype=np.uint8)), up(np.arange(B, dtype=np.int32))
    adv, tgt = up(rng.standard_normal(B).astype(np.float32)), up(rng.standard_normal(B).astype(np.float32))
    hot = up(np.eye(A_DIM, dtype=np.float32)[rng.integers(0, A_DIM, B)])
    state = {"it": 0}

    def impala_step():
        net.keras_impala_step(obs, idx, adv, hot, tgt, 0.01)
        net.adam_keras(3e-4, state["it"], clipnorm=40.0)
        state["it"] += 1

    def replay(double):
        alg = algs[double]
        return lambda: alg.actor.train_replay(alg.target_actor, alg.buff, slots[double], dqn_mod.GAMMA, double)

    def replay_per(double):
        alg = pers[double]
        return lambda: alg.actor.train_replay_per(alg.target_actor, alg.buff, draws, alg.per_beta(), dqn_mod.GAMMA, double)

    def replay_nstep():
        return nstep.actor.train_replay(nstep.target_actor, nstep.buff, nstep_slots, dqn_mod.GAMMA, False)

    def replay_nstep_per():
        return nstep_per.actor.train_replay_per(nstep_per.target_actor, nstep_per.buff, draws, nstep_per.per_beta(),
                                                dqn_mod.GAMMA, False)

    msg_rng = np.random.default_rng(3)
    msg = {"cur_state": _states(msg_rng, 20), "next_state": _states(msg_rng, 20),
           "action": msg_rng.integers(0, A_DIM, 20), "reward": msg_rng.choice([-1.0, 0.0, 1.0], 20),
           "done": msg_rng.random(20) < 0.02}

    def ingest(alg):
        def fn():
            alg.prepare_data(msg)
            torch.cuda.synchronize()
        return fn

    cases = [("DQN.train (loss read back)", algs[False].train), ("DQN.train, PER (loss read back)", pers[False].train),
             ("DQN.train, n_step 3 (loss read back)", nstep.train),
             ("DQN.train, PER, n_step 3 (loss read back)", nstep_per.train),
             ("DQN.train, double_dqn (loss read back)", algs[True].train),
             ("DQN.train, PER, double_dqn (loss read back)", pers[True].train),
             ("dqn step + adam, enqueue only", replay(False)), ("dqn step + adam, PER, enqueue only", replay_per(False)),
             ("dqn step + adam, n_step 3, enqueue only", replay_nstep),
             ("dqn step + adam, PER, n_step 3, enqueue only", replay_nstep_per),
             ("dqn step + adam, double_dqn, enqueue only", replay(True)),
             ("dqn step + adam, PER, double_dqn, enqueue only", replay_per(True)),
             ("prepare_data, 20 rows, synchronised", ingest(algs[False])),
             ("prepare_data, 20 rows, PER, synchronised", ingest(pers[False])),
             ("keras_impala_step + adam_keras, 32 rows, enqueue only", impala_step)]
    if args.model == "DqnMlp":
        cases = cases[:-1]                                  # (the IMPALA row is the CNN trunk's)
    pos = 12                                                # the head arms go behind the twelve train rows
    heads = [(key, count, duel) for key, count in (("atoms", args.atoms), ("quantiles", args.quantiles))
             for duel in ((False, True) if args.dist_dueling else (False,))]
    for key, count, duel in heads:
        if count <= 1:
            continue
        # the distributional arms share ONE algorithm per (PER, n_step) -- double_dqn is an argument of the train and the
        # kernel selection a switch of the two nets -- so four more rings, not sixteen
        dist = {(per, n): build_dqn(False, args.capacity, per, n, dist_dueling=duel, **{key: count})
                for per in (False, True) for n in (1, 3)}
        dist_slots = torch.tensor(dist[(False, 1)].buff.sample(B), dtype=torch.int32).cuda()

        def dist_case(per, n, double, wide, read_back, dist=dist, dist_slots=dist_slots):
            alg = dist[(per, n)]

            def fn():
                alg.double_dqn = double
                for net in (alg.actor.net, alg.target_actor.net):
                    net.set_dist_wide(wide)
                if read_back:
                    return alg.train()
                if per:
                    return alg.actor.train_replay_per(alg.target_actor, alg.buff, draws, alg.per_beta(), dqn_mod.GAMMA, double)
                return alg.actor.train_replay(alg.target_actor, alg.buff, dist_slots, dqn_mod.GAMMA, double)
            return fn
        extra = []
        for read_back in (True, False):
            for wide in (True, "forward", False) if duel else (True, False):
                for per, n, double in ((False, 1, False), (True, 1, False), (False, 3, False), (True, 3, False),
                                       (False, 1, True), (True, 1, True), (False, 3, True), (True, 3, True)):
                    name = "{}, {} {}{}{}{}{}{}{}".format(
                        "DQN.train" if read_back else "dqn step + adam", key, count, ", dist_dueling" if duel else "",
                        ", PER" if per else "", ", n_step 3" if n == 3 else "", ", double_dqn" if double else "",
                        {True: "", "forward": ", generic d(features)", False: ", generic head kernels"}[wide],
                        " (loss read back)" if read_back else ", enqueue only")
                    extra.append((name, dist_case(per, n, double, wide, read_back)))
        cases = cases[:pos] + extra + cases[pos:]
        pos += len(extra)
    if args.noisy:
        noisy = {d: build_dqn(d, args.capacity, noisy=True) for d in (False, True)}
        noisy_slots = {d: torch.tensor(a.buff.sample(B), dtype=torch.int32).cuda() for d, a in noisy.items()}

        def noisy_replay(double):
            alg = noisy[double]
            return lambda: alg.actor.train_replay(alg.target_actor, alg.buff, noisy_slots[double], dqn_mod.GAMMA, double)

        def noisy_launches():
            online, target = noisy[False].actor.net, noisy[False].target_actor.net
            online.compose(state["it"], 0)
            target.compose(state["it"], 1)
            online.noisy_grads()

        extra = [("DQN.train, noisy (loss read back)", noisy[False].train),
                 ("DQN.train, noisy, double_dqn (loss read back)", noisy[True].train),
                 ("dqn step + adam, noisy, enqueue only", noisy_replay(False)),
                 ("dqn step + adam, noisy, double_dqn, enqueue only", noisy_replay(True)),
                 ("compose online + compose target + noisy_grads alone, enqueue only", noisy_launches)]
        cases = cases[:pos] + extra + cases[pos:]
        pos += len(extra)
    for _, fn in cases:
        for _ in range(20):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in cases}
    for _ in range(args.windows):
        for name, fn in cases:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.trains):
                fn()
            torch.cuda.synchronize()
            times[name].append(1e6 * (time.perf_counter() - t0) / args.trains)
    lines = ["| what ({}, A = 4, B = 32) | us per call: median | min | max |".format(
        "DqnCnn 84x84x4" if args.model == "DqnCnn" else "DqnMlp, state 4"), "|---|---|---|---|"]
    for name, _ in cases:
        t = sorted(times[name])
        lines.append("| {} | {:.1f} | {:.1f} | {:.1f} |".format(name, t[len(t) // 2], t[0], t[-1]))
    text = "\n".join(lines)
    print(text)
    print("device:", torch.cuda.get_device_name(0), "| windows", args.windows, "x", args.trains, "calls | ring capacity",
          args.capacity)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n\ndevice: {} | {} windows x {} calls | ring capacity {}\n".format(
                torch.cuda.get_device_name(0), args.windows, args.trains, args.capacity))


if __name__ == "__main__":
    main()
