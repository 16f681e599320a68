"""GPU tests of the DQN path: ``xt_replay_gather`` (bit-exact, offsets beyond 2^32), ``xt_dqn_loss`` and
``xt_net_dqn_step`` against the float64 checker of tests/dqn_helpers.py, and the algorithm through
``alg_builder("DQN")`` (ring wrap-around, target cadence, short buffer, save / restore, CPU replica)."""
import collections
import random

import numpy as np
import pytest
import torch

import dqn_helpers as H

pytestmark = pytest.mark.gpu

GAMMA = 0.99


@pytest.fixture(scope="module")
def L():
    from xingtian_amd import lib
    lib.require_gpu()
    lib.load()
    return lib


@pytest.fixture(autouse=True)
def _module_constants_restored():
    """import_config overrides the modules' constants for the rest of the process: put them back"""
    from xingtian_amd.algorithm.dqn import dqn
    from xingtian_amd.model.dqn import dqn_cnn, dqn_mlp
    saved = [(m, {k: v for k, v in vars(m).items() if k.isupper()}) for m in (dqn, dqn_cnn, dqn_mlp)]
    yield
    torch.cuda.synchronize()
    for m, consts in saved:
        vars(m).update(consts)


# ------------------------------------------------------------------------------------------------ xt_replay_gather
@pytest.mark.parametrize("row_bytes", [16, 28224])
@pytest.mark.parametrize("b", [1, 33])
def test_replay_gather_is_bit_exact_for_duplicate_and_unsorted_slots(L, row_bytes, b):
    rng = np.random.default_rng(row_bytes + b)
    ring = torch.from_numpy(rng.integers(0, 256, (40, row_bytes), dtype=np.uint8)).cuda()
    slots = rng.integers(0, 40, b)
    if b > 1:
        slots[:4] = [39, 0, 39, 7]                                   # unsorted, one duplicate, both ends of the ring
        assert len(set(slots.tolist())) < b
    rc, dst = H.gpu_replay_gather(ring, torch.from_numpy(slots.astype(np.int32)).cuda())
    assert rc == 0
    assert torch.equal(dst, ring[torch.from_numpy(slots).cuda()])


def test_replay_gather_addresses_rows_beyond_two_and_four_gigabytes(L):
    """a ring of 160 000 rows x 28 224 B (4.5 GB, uninitialised but for the rows read): byte offsets below 2^31, above
    2^31 and above 2^32"""
    cap, rb = 160000, 28224
    slots = [0, 76100, 152200, 159999]
    offs = [s * rb for s in slots]
    assert offs[0] < 2 ** 31 < offs[1] < 2 ** 32 < offs[2] < offs[3]
    ring = torch.empty((cap, rb), dtype=torch.uint8, device="cuda")
    rng = np.random.default_rng(3)
    rows = torch.from_numpy(rng.integers(0, 256, (len(slots), rb), dtype=np.uint8)).cuda()
    for s, r in zip(slots, rows):
        ring[s] = r
    order = [2, 0, 3, 1, 2]
    rc, dst = H.gpu_replay_gather(ring, torch.tensor([slots[i] for i in order], dtype=torch.int32, device="cuda"))
    assert rc == 0 and torch.equal(dst, rows[torch.tensor(order, device="cuda")])
    del ring
    torch.cuda.empty_cache()


def test_replay_gather_refuses_rows_that_are_no_multiple_of_16_bytes(L):
    ring = torch.zeros((4, 32), dtype=torch.uint8, device="cuda")
    slots = torch.zeros(2, dtype=torch.int32, device="cuda")
    for kw in (dict(row_bytes=20), dict(row_bytes=0), dict(b=0), dict(capacity=0)):
        rc, dst = H.gpu_replay_gather(ring, slots, **kw)
        assert rc != 0 and bool((dst == 0xA5).all()), kw            # an error, and nothing was launched
    rc, _ = H.gpu_replay_gather(ring, slots, row_bytes=20)
    assert "multiple of 16" in L.load().xt_last_error().decode()
    # a slot outside the ring is not read: a zero row
    rc, dst = H.gpu_replay_gather(ring + 7, torch.tensor([1, 4, -1], dtype=torch.int32, device="cuda"))
    assert rc == 0 and bool((dst[0] == 7).all()) and not bool(dst[1:].any())


# ------------------------------------------------------------------------------------------------ xt_dqn_loss
def _loss_inputs(b, a, seed, done_mode):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    d = dict(logits=f(b, a), value=f(b), t_logits=f(b, a) * 2, t_value=f(b), o_logits=f(b, a) * 2, o_value=f(b),
             action=rng.integers(0, a, b).astype(np.int32), reward=rng.standard_normal(b))
    d["done"] = {"all": np.ones(b, np.uint8), "none": np.zeros(b, np.uint8),
                 "mixed": (np.arange(b) % 3 == 0).astype(np.uint8) * np.uint8(1 + (seed % 2) * 254)}[done_mode]   # truthiness: 1 or 255
    return d


def _check_loss(got, d, dueling, double):
    f64 = lambda x: None if x is None else np.asarray(x, np.float64)
    ref = H.dqn_loss_ref(f64(d["logits"]), f64(d["value"]), f64(d["t_logits"]), f64(d["t_value"]),
                         f64(d["o_logits"]) if double else None, f64(d["o_value"]) if double else None,
                         d["action"], d["reward"], d["done"], GAMMA, dueling)
    b = len(d["action"])
    assert np.array_equal(got["astar"], ref["astar"])                                      # exact
    assert np.array_equal(got["y"], H.y_numpy1(d["reward"], got["maxq"], d["done"], GAMMA))  # bit-exact from its own maxq
    assert H.rel_max(got["maxq"], ref["maxq"]) <= 1e-5
    out = got["out"]
    print("dqn_loss: loss", out[0], ref["loss"], "| dlogits", H.rel_max(got["dlogits"], ref["dlogits"]))
    assert abs(out[0] - ref["loss"]) <= 1e-4 * abs(ref["loss"])
    assert abs(out[1] - ref["abs_td"]) <= 1e-5 * max(1.0, ref["abs_td"])
    assert abs(out[2] - ref["mean_maxq"]) <= 1e-5 * max(1.0, abs(ref["mean_maxq"]))
    assert H.rel_max(got["dlogits"], ref["dlogits"]) <= 1e-5
    if dueling:
        assert H.rel_max(got["dvalue"], ref["dvalue"]) <= 1e-5
    else:
        assert not got["dvalue"].any() and got["dvalue"].shape == (b,)                      # exactly 0
    return ref


@pytest.mark.parametrize("done_mode", ["all", "none", "mixed"])
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("dueling", [False, True])
@pytest.mark.parametrize("b,a", [(1, 2), (32, 4), (33, 18), (7, 64)])
def test_dqn_loss_against_float64(L, b, a, dueling, double, done_mode):
    d = _loss_inputs(b, a, 100 * b + a + 2 * dueling + double, done_mode)
    rc, got = H.gpu_dqn_loss(d["logits"], d["value"], d["t_logits"], d["t_value"], d["o_logits"] if double else None,
                             d["o_value"] if double else None, d["action"], d["reward"], d["done"], GAMMA, dueling)
    assert rc == 0
    _check_loss(got, d, dueling, double)


@pytest.mark.parametrize("dueling", [False, True])
def test_dqn_loss_ties_take_the_first_index_and_double_dqn_picks_with_the_online_net(L, dueling):
    b, a = 6, 5
    d = _loss_inputs(b, a, 11, "none")
    d["t_logits"][0] = 1.25                                            # all equal -> index 0
    d["t_logits"][1] = [0.5, 2.0, -1.0, 2.0, 2.0]                      # three maxima -> index 1
    d["t_logits"][2] = [-3.0, -3.0, -1.0, -2.0, -1.0]                  # two maxima -> index 2
    d["o_logits"][:] = -d["t_logits"]                                  # the online net prefers what the target net likes least
    d["o_logits"][3] = [0.0, 7.0, 7.0, 1.0, 0.0]                       # ... and ties too -> index 1
    for double in (False, True):
        rc, got = H.gpu_dqn_loss(d["logits"], d["value"], d["t_logits"], d["t_value"], d["o_logits"] if double else None,
                                 d["o_value"] if double else None, d["action"], d["reward"], d["done"], GAMMA, dueling)
        assert rc == 0
        ref = _check_loss(got, d, dueling, double)
        if double:
            assert list(got["astar"][:4]) == [0, 2, 0, 1]
            plain = np.argmax(H.q_from_heads(d["t_logits"].astype(np.float64), d["t_value"], dueling), 1)
            assert (got["astar"] != plain).sum() >= 3                  # online and target argmax differ
            q_t = H.q_from_heads(d["t_logits"].astype(np.float64), d["t_value"], dueling)
            assert (ref["maxq"] < q_t.max(axis=1) - 1e-3).any()        # ... so maxq is not the target net's maximum
        else:
            assert list(got["astar"][:3]) == [0, 1, 2]


def test_dqn_loss_gathers_the_label_rings_through_slots_and_accumulates(L):
    b, a, n = 9, 4, 30
    d = _loss_inputs(n, a, 5, "mixed")
    slots = np.random.default_rng(1).permutation(n)[:b].astype(np.int32)
    head = {k: d[k][:b] for k in ("logits", "value", "t_logits", "t_value")}
    acc = torch.tensor([2.0, 5.0], device="cuda")
    rc, got = H.gpu_dqn_loss(head["logits"], head["value"], head["t_logits"], head["t_value"], None, None, d["action"],
                             d["reward"], d["done"], GAMMA, True, slots=slots, acc=acc)
    assert rc == 0
    sub = dict(head, action=d["action"][slots], reward=d["reward"][slots], done=d["done"][slots], o_logits=None, o_value=None)
    _check_loss(got, sub, True, False)
    acc = acc.cpu().numpy()
    assert acc[0] == np.float32(2.0) + got["out"][0] and acc[1] == 6.0


def test_dqn_loss_refuses_bad_sizes_and_launches_nothing(L):
    d = _loss_inputs(4, 65, 0, "none")
    for kw in (dict(a=65), dict(b=0)):
        rc, got = H.gpu_dqn_loss(d["logits"], d["value"], d["t_logits"], d["t_value"], None, None, d["action"], d["reward"],
                                 d["done"], GAMMA, False, **kw)
        assert rc != 0
        assert np.isnan(got["dlogits"]).all() and np.isnan(got["out"]).all() and (got["astar"] == -1).all()
        assert "xt_dqn_loss" in L.load().xt_last_error().decode()


# ------------------------------------------------------------------------------------------------ xt_net_dqn_step
def _spec_pair(kind, a_dim, dueling):
    from xingtian_amd.model import netspec
    if kind == "cnn":
        return netspec.dqn_cnn((84, 84, 4), a_dim, dueling), H.oracle_spec("cnn", (84, 84, 4), a_dim)
    return netspec.dqn_mlp((4,), a_dim, 32, 1, dueling), H.oracle_spec("mlp", (4,), a_dim, 32, 1)


def _states(kind, rng, n):
    if kind == "cnn":
        return rng.integers(0, 256, (n, 84, 84, 4), dtype=np.uint8)
    return rng.standard_normal((n, 4)).astype(np.float32)


def _assert_step(got_loss, grads, ref, spec, ospec, dueling):
    assert abs(got_loss - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"])), (got_loss, ref["loss"])
    worst = 0.0
    for h, o in H.name_map(spec, ospec).items():
        r = ref["grads"][o]
        err = np.linalg.norm(grads[h].reshape(r.shape) - r) / (np.linalg.norm(r) + 1e-30)
        worst = max(worst, err)
        assert err <= 1e-5, (h, err)
    print("dqn step: loss", got_loss, float(ref["loss"]), "| worst gradient tensor", worst)
    if not dueling:
        v = ospec["v_name"]
        assert not ref["grads"][v + "/kernel"].any() and not ref["grads"][v + "/bias"].any()


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("dueling", [False, True])
@pytest.mark.parametrize("b", [5, 32])
@pytest.mark.parametrize("kind", ["mlp", "cnn"])
def test_net_dqn_step_against_float64(L, kind, b, dueling, double):
    from xingtian_amd.model.hip_net import HipActorCritic
    a_dim = 2 if kind == "mlp" else 4
    spec, ospec = _spec_pair(kind, a_dim, dueling)
    rng = np.random.default_rng(b + 2 * dueling + double)
    p_on, p_tg = H.seeded_params(ospec, 1, dueling), H.seeded_params(ospec, 2, dueling)
    net, target = HipActorCritic(spec, max_batch=32, seed=0), HipActorCritic(spec, max_batch=32, seed=0)
    net.set_weights(H.to_keras_names(spec, ospec, p_on))
    target.set_weights(H.to_keras_names(spec, ospec, p_tg))
    target_before = target.params.clone()
    cap = 40
    cur, nxt = _states(kind, rng, cap), _states(kind, rng, cap)
    action, reward = rng.integers(0, a_dim, cap).astype(np.int32), rng.standard_normal(cap)
    done = (rng.random(cap) < 0.3).astype(np.uint8)
    slots = rng.permutation(cap)[:b].astype(np.int32)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = net.dqn_step(target, net.to_device_obs(cur), net.to_device_obs(nxt), up(slots), up(action), up(reward), up(done),
                       GAMMA, dueling, double)
    torch.cuda.synchronize()
    orc = H.DqnOracle(ospec, p_on, p_tg, dueling, double, GAMMA, lr=3e-4, dtype=np.float64)
    ref = orc.step(cur[slots], nxt[slots], action[slots], reward[slots], done[slots], apply=False)
    _assert_step(float(out.cpu().numpy()[0]), net.grads_dict(), ref, spec, ospec, dueling)
    # the hidden 1-wide head: zero gradient, and the optimiser never touches its parameters
    v0, v1 = spec.v_off, spec.v_off + spec.feat + 1
    before = net.params[v0:v1].clone()
    flat_before = net.params.clone()
    if not dueling:
        assert not bool(net.grads[v0:v1].any()) and not bool(before.any())
    net.adam_keras(3e-4, 0, clipnorm=10.0 if kind == "cnn" else 0.0)
    torch.cuda.synchronize()
    assert not torch.equal(net.params, flat_before)
    if not dueling:
        assert torch.equal(net.params[v0:v1], before)                  # bitwise unchanged
    assert torch.equal(target.params, target_before) and not bool(target.grads.any())     # the target net is forward only


def test_net_dqn_step_refusals(L):
    from xingtian_amd.model import netspec
    from xingtian_amd.model.hip_net import HipActorCritic
    spec = netspec.dqn_mlp((4,), 2, 32, 1, False)
    net, target = HipActorCritic(spec, max_batch=8, seed=0), HipActorCritic(spec, max_batch=8, seed=0)
    other = HipActorCritic(netspec.dqn_mlp((4,), 3, 32, 1, False), max_batch=8, seed=0)
    ring = torch.zeros((10, 4), dtype=torch.float32, device="cuda")
    lab = (torch.zeros(10, dtype=torch.int32, device="cuda"), torch.zeros(10, dtype=torch.float64, device="cuda"),
           torch.zeros(10, dtype=torch.uint8, device="cuda"))
    slots = torch.zeros(4, dtype=torch.int32, device="cuda")
    for tgt, rg, sl, word in ((net, ring, slots, "own parameter buffers"), (other, ring, slots, "same description"),
                              (target, ring, torch.zeros(9, dtype=torch.int32, device="cuda"), "batch"),
                              (target, torch.zeros((10, 8), dtype=torch.float32, device="cuda"), slots, "row_bytes")):
        with pytest.raises(RuntimeError) as info:
            net.dqn_step(tgt, rg, rg, sl, *lab, GAMMA, False, False)
        assert word in str(info.value), (word, str(info.value))
    net.set_dp(0, 2)
    with pytest.raises(RuntimeError) as info:
        net.dqn_step(target, ring, ring, slots, *lab, GAMMA, False, False)
    assert "data parallelism" in str(info.value)


DQN_ENTRIES = ("xt_net_dqn_step", "xt_net_dqn_step_per", "xt_net_dqn_step_n", "xt_net_dqn_step_dist")


def _dispatch_case(per, follow, dist):
    """-> (net with a counting lib, positional arguments of ``dqn_step`` up to double_dqn, its keywords, trees or None):
    DqnMlp state 4, hidden 32, A = 2 (atoms 3 if ``dist``), ring capacity 50, B = 4"""
    import nstep_helpers as N
    import per_helpers as P
    from xingtian_amd.model import netspec
    from xingtian_amd.model.hip_net import HipActorCritic
    cap, b, a_dim, atoms = 50, 4, 2, 3
    spec = netspec.dqn_mlp((4,), a_dim, 32, 1, False, atoms if dist else 1)
    net, target = HipActorCritic(spec, max_batch=b, seed=0), HipActorCritic(spec, max_batch=b, seed=1)
    if dist:
        net.set_dist(atoms, -10.0, 10.0)
        target.set_dist(atoms, -10.0, 10.0)
    rng = np.random.default_rng(4 * per + 2 * follow + dist)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    cur, nxt = net.to_device_obs(_states("mlp", rng, cap)), net.to_device_obs(_states("mlp", rng, cap))
    labels = (up(rng.integers(0, a_dim, cap).astype(np.int32)), up(rng.standard_normal(cap)),
              up((rng.random(cap) < 0.1).astype(np.uint8)))
    kw, t = dict(dist=dist), None
    if follow:                                                           # messages of five rows
        kw.update(follow=up((4 - np.arange(cap) % 5).astype(np.int32)), n=3)
    if per:
        t = P.GpuTrees(cap, 0.6)
        assert t.add(0, cap) == 0
        kw.update(per=dict(size=cap, u=up(rng.random(b)), sum_tree=t.sum, min_tree=t.min, max_prio=t.max_prio, alpha=0.6,
                           beta=0.4, eps=1e-6))
    slots = None if per else up(rng.permutation(cap)[:b].astype(np.int32))
    net.lib = N.CountingLib(net.lib)
    net.grads.zero_()
    return net, (target, cur, nxt, slots, *labels, GAMMA, False, False), kw, t


@pytest.mark.parametrize("dist", [False, True])
@pytest.mark.parametrize("follow", [False, True])
@pytest.mark.parametrize("per", [False, True])
def test_net_dqn_step_reaches_the_entry_its_arguments_name(L, per, follow, dist):
    """the dispatch table of ``HipActorCritic.dqn_step``: dist, else follow, else per, else the plain entry"""
    net, args, kw, _ = _dispatch_case(per, follow, dist)
    out = net.dqn_step(*args, **kw)
    torch.cuda.synchronize()
    want = DQN_ENTRIES[3 if dist else 2 if follow else 1 if per else 0]
    assert {e: net.lib.calls[e] for e in DQN_ENTRIES} == {e: int(e == want) for e in DQN_ENTRIES}
    assert out is net.loss_out and bool(torch.isfinite(out).all())
    assert bool(net.grads.any())
    assert hasattr(net, "nstep_boot") == follow and hasattr(net, "per_slots") == per


@pytest.mark.parametrize("name", ["dqn_step_per", "dqn_step_n", "dqn_step_dist"])
def test_net_dqn_step_earlier_names_forward_to_it(L, name):
    """``dqn_step_per`` / ``dqn_step_n`` / ``dqn_step_dist`` with their old argument order are ``dqn_step``: the same C
    entry and, for the two that move no priority tree here, the same bits in ``loss_out`` and the gradient"""
    per, follow, dist = name == "dqn_step_per", name == "dqn_step_n", name == "dqn_step_dist"
    net, args, kw, t = _dispatch_case(per, follow, dist)
    first = net.dqn_step(*args, **kw).clone()
    grads = net.grads.clone()
    net.grads.zero_()
    target, cur, nxt, slots, action, reward, done = args[:7]
    if per:
        again = net.dqn_step_per(target, cur, nxt, 50, kw["per"]["u"], action, reward, done, GAMMA, False, False, t.sum, t.min,
                                 t.max_prio, 0.6, 0.4, 1e-6)
    elif follow:
        again = net.dqn_step_n(target, cur, nxt, slots, action, reward, done, kw["follow"], 3, GAMMA, False, False)
    else:
        again = net.dqn_step_dist(target, cur, nxt, slots, action, reward, done, GAMMA, False)
    torch.cuda.synchronize()
    want = "xt_net_" + name
    assert {e: net.lib.calls[e] for e in DQN_ENTRIES} == {e: 2 * int(e == want) for e in DQN_ENTRIES}
    assert again is net.loss_out and bool(torch.isfinite(again).all()) and bool(net.grads.any())
    if not per:
        assert torch.equal(again.view(torch.int32), first.view(torch.int32))
        assert torch.equal(net.grads.view(torch.int32), grads.view(torch.int32))


# ------------------------------------------------------------------------------------------------ alg_builder("DQN")
def _messages(kind, rng, a_dim, n_msg=3, rows=20):
    msgs = []
    for _ in range(n_msg):
        msgs.append({"cur_state": _states(kind, rng, rows), "next_state": _states(kind, rng, rows),
                     "action": rng.integers(0, a_dim, rows).astype(np.int32),
                     "reward": [float(x) for x in rng.standard_normal(rows)],
                     "done": [bool(x) for x in rng.random(rows) < 0.3]})
    return msgs


def _build(kind, a_dim, dueling, double, batch, buffer_size=50, freq=3):
    from xingtian_amd.algorithm import alg_builder
    mc = {"dueling": dueling, "SEED": 3, "LR": 3e-4}
    if kind == "mlp":
        mc.update(HIDDEN_SIZE=32, NUM_LAYERS=1)
    info = {"actor": {"model_name": "DqnCnn" if kind == "cnn" else "DqnMlp", "type": "learner",
                      "state_dim": [84, 84, 4] if kind == "cnn" else [4], "action_dim": a_dim, "model_config": mc}}
    cfg = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1, "BUFFER_SIZE": buffer_size,
           "BATCH_SIZE": batch, "TARGET_UPDATE_FREQ": freq, "GAMMA": GAMMA, "double_dqn": double}
    return alg_builder("DQN", info, cfg), info


def _feed(alg, msgs, dq=None):
    for m in msgs:
        alg.prepare_data(m)
        if dq is not None:
            dq.extend(zip(m["cur_state"], m["next_state"], m["action"], m["reward"], m["done"]))


def _batch(dq, logical):
    rows = [dq[i] for i in logical]
    return [np.stack([r[k] for r in rows]) if k < 2 else np.asarray([r[k] for r in rows]) for k in range(5)]


@pytest.mark.parametrize("kind,dueling,double,batch", [("mlp", True, True, 32), ("cnn", False, False, 8)])
def test_dqn_algorithm_four_trains_target_cadence_restore_and_replica(L, tmp_path, kind, dueling, double, batch):
    a_dim = 2 if kind == "mlp" else 4
    spec, ospec = _spec_pair(kind, a_dim, dueling)
    alg, info = _build(kind, a_dim, dueling, double, batch)
    assert alg.device_step and alg.buff.cur_state is None
    rng = np.random.default_rng(17)
    msgs, dq = _messages(kind, rng, a_dim), collections.deque(maxlen=50)
    _feed(alg, msgs, dq)
    assert alg.buff.size() == 50 == len(dq) and alg.buff.head == 10             # 60 rows into 50 slots: wrapped
    p_on, p_tg = H.seeded_params(ospec, 1, dueling), H.seeded_params(ospec, 2, dueling)
    w_on, w_tg = H.to_keras_names(spec, ospec, p_on), H.to_keras_names(spec, ospec, p_tg)
    alg.actor.set_weights(w_on)
    alg.target_actor.set_weights(w_tg)
    clip = 10.0 if kind == "cnn" else None
    orc = H.DqnOracle(ospec, p_on, p_tg, dueling, double, GAMMA, 3e-4, clip, np.float64)
    orc32 = H.DqnOracle(ospec, {k: v.copy() for k, v in p_on.items()}, {k: v.copy() for k, v in p_tg.items()}, dueling,
                        double, GAMMA, 3e-4, clip, np.float32)
    samples = [rng.permutation(50)[:batch] for _ in range(4)]
    target_init = alg.target_actor.net.params.clone()
    saved = None
    for t, logical in enumerate(samples, 1):
        loss = alg.train_on_slots(alg.buff.slots_of(logical))
        assert isinstance(loss, float)
        if t == 1:                                                               # the single-step bars
            ref = orc.step(*_batch(dq, logical), apply=False)
            _assert_step(loss, alg.actor.net.grads_dict(), ref, spec, ospec, dueling)
        for o in (orc, orc32):
            o.step(*_batch(dq, logical))
            if t % 3 == 0:
                o.sync_target()
        tp = alg.target_actor.net.params
        if t < 3:
            assert torch.equal(tp, target_init)                                  # bitwise the initial ones
        elif t == 3:
            assert torch.equal(tp, alg.actor.net.params) and not torch.equal(tp, target_init)
            saved = alg.save(str(tmp_path), 1)[0]
        else:
            assert not torch.equal(tp, alg.actor.net.params)
    assert alg.train_count == 4 and alg.actor.iterations == 4
    # four trains: every tensor within 3x the float32 oracle's own drift from float64
    w4, report = alg.get_weights(), {}
    for h, o in H.name_map(spec, ospec).items():
        r = orc.net.params[o]
        d64 = r - np.asarray(p_on[o], np.float64)
        nrm = np.linalg.norm(d64) + 1e-30
        gpu = np.linalg.norm(w4[h].reshape(r.shape) - np.asarray(p_on[o], np.float64) - d64) / nrm
        f32 = np.linalg.norm(orc32.net.params[o].astype(np.float64) - np.asarray(p_on[o], np.float64) - d64) / nrm
        report[h] = (float(gpu), float(f32))
    print("dqn four trains, per tensor (gpu, oracle32) deviation of the weight change:", report)
    for h, (gpu, f32) in report.items():
        assert gpu <= 3.0 * f32, (h, gpu, f32)
    # save after train 3 -> fresh algorithm -> restore -> train 4 bitwise equals the uninterrupted run's
    alg2, _ = _build(kind, a_dim, dueling, double, batch)
    alg2.restore(model_name=saved)
    assert alg2.actor.iterations == 3 and torch.equal(alg2.actor.net.params, alg2.target_actor.net.params)
    _feed(alg2, msgs)
    loss2 = alg2.train_on_slots(alg2.buff.slots_of(samples[3]))
    assert loss2 == loss and torch.equal(alg2.actor.net.params, alg.actor.net.params)
    assert set(np.load(saved).files) >= set(spec.names) | {"keras_adam_iterations"}
    # the learner's weights in a CPU replica
    from xingtian_amd.model import model_builder
    rep_info = dict(info["actor"], type="explorer", model_config=dict(info["actor"]["model_config"], DEVICE="cpu"))
    replica = model_builder(rep_info)
    replica.set_weights(alg.get_weights())
    states = _states(kind, rng, 8)
    q_gpu, q_cpu = alg.actor.predict(states), replica.predict(states)
    assert q_gpu.dtype == q_cpu.dtype == np.float32 and q_gpu.shape == (8, a_dim)
    scale = max(1.0, np.abs(q_gpu).max())
    assert np.abs(q_gpu - q_cpu).max() <= 1e-5 * scale


def test_dqn_train_on_a_buffer_shorter_than_the_batch_uses_every_row(L):
    kind, a_dim = "mlp", 2
    spec, ospec = _spec_pair(kind, a_dim, True)
    alg, _ = _build(kind, a_dim, True, False, batch=32)
    rng = np.random.default_rng(5)
    msgs, dq = _messages(kind, rng, a_dim, n_msg=1, rows=5), collections.deque(maxlen=50)
    _feed(alg, msgs, dq)
    p_on, p_tg = H.seeded_params(ospec, 1, True), H.seeded_params(ospec, 2, True)
    alg.actor.set_weights(H.to_keras_names(spec, ospec, p_on))
    alg.target_actor.set_weights(H.to_keras_names(spec, ospec, p_tg))
    random.seed(9)
    logical = random.sample(range(5), 5)
    random.seed(9)
    loss = alg.train()
    ref = H.DqnOracle(ospec, p_on, p_tg, True, False, GAMMA, 3e-4).step(*_batch(dq, logical), apply=False)
    _assert_step(loss, alg.actor.net.grads_dict(), ref, spec, ospec, True)
    assert alg.train_count == 1


def test_device_replay_refuses_rings_larger_than_free_memory_naming_the_bytes(L):
    from xingtian_amd.algorithm.dqn.dqn import DeviceReplay
    free, _ = torch.cuda.mem_get_info()
    cap = free // (2 * 28224) + 1000
    ring = DeviceReplay(cap, "cuda:0")
    z = np.zeros((1, 84, 84, 4), np.uint8)
    with pytest.raises(RuntimeError) as info:
        ring.add(z, z, [0], [0.0], [False])
    assert str(cap * (2 * 28224 + 13)) in str(info.value) and ring.cur_state is None
