"""GPU tests of prioritised replay: the tree kernels (``xt_per_add`` / ``xt_per_update`` / ``xt_per_sample``) on the
recorded cases of tests/golden/per_cases.npz against the restatement of tests/per_helpers.py, the weighted head
(``xt_dqn_loss_w``), ``xt_net_dqn_step_per`` against the float64 checker, and ``alg_builder("DQN")`` with
``prioritized_replay``."""
import math
import random

import numpy as np
import pytest
import torch

import dqn_helpers as H
import per_helpers as P

pytestmark = pytest.mark.gpu

GAMMA = 0.99
EPS = 1e-6
NAMES = ("c5", "c37", "c707", "c1000", "c64", "c37_alpha1", "c37_beta1", "c64_edge")


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


@pytest.fixture(scope="module")
def cases(golden_dir):
    return P.load_cases(golden_dir)


def device_priority(p):
    """the priority the device forms from a recorded one: the TD error goes through float32"""
    return float(np.float32(p)) + EPS


@pytest.fixture(scope="module")
def replayed(L, cases):
    """name -> (GpuTrees after the case's whole script, its read-back): each script runs once for the module"""
    done = {}

    def get(name):
        if name not in done:
            c = cases[name]
            t = P.GpuTrees(c.capacity, c.alpha)
            for step in c.steps():
                if step[0] == "add":
                    for first, count in step[1]:
                        assert t.add(first, count) == 0
                else:
                    sign = [1.0 if i % 2 else -1.0 for i in range(len(step[1]))]        # |delta| is what counts
                    assert t.update(step[1], np.float32(step[2]) * np.float32(sign), EPS, stride=2) == 0
            done[name] = (t, t.read())
        return done[name]
    return get


# ------------------------------------------------------------------------------------------------ trees
@pytest.mark.parametrize("name", NAMES)
def test_trees_after_the_recorded_adds_and_updates(cases, replayed, name):
    c = cases[name]
    _, (s, m, max_prio) = replayed(name)
    leaves, host_max = c.host_leaves(device_priority)
    assert max_prio == host_max                                            # exactly
    got = np.asarray(s[c.cap2:])
    written = np.asarray(leaves) != 0.0
    assert written.sum() == c.n and not got[~written].any() and all(math.isinf(x) for x in np.asarray(m[c.cap2:])[~written])
    err = P.rel_err(got[written], np.asarray(leaves)[written])
    print("per trees", name, "leaves rel", err)
    assert err <= 1e-12
    assert s[c.cap2:] == [0.0 if math.isinf(x) else x for x in m[c.cap2:]]  # both trees hold the same leaves
    P.assert_trees_follow_from_their_leaves(s, m)


def test_the_recorded_update_batches_cover_the_batch_sizes(cases):
    sizes = {len(b[0]) for c in cases.values() for b in c.batches}
    assert {1, 32, 33, 256} <= sizes
    assert any(len(set(b[0])) < len(b[0]) for c in cases.values() for b in c.batches)      # duplicates within a batch


def test_update_with_duplicate_slots_keeps_the_last_occurrence_and_every_priority_counts_for_the_maximum(L):
    t = P.GpuTrees(5, 0.6)
    assert t.add(3, 2) == 0 and t.add(0, 3) == 0                           # a wrapping message: two calls
    slots = [3, 1, 3, 3, 0, 1]
    delta = np.float32([9.5, -0.25, 2.0, -0.5, 1.5, 0.75])                 # the largest |delta| belongs to a loser
    assert t.update(slots, delta, 1e-3, stride=2) == 0
    s, m, max_prio = t.read()
    prio = lambda d: float(abs(np.float32(d))) + 1e-3
    assert max_prio == prio(9.5)
    want = {3: prio(-0.5), 1: prio(0.75), 0: prio(1.5), 2: 1.0, 4: 1.0}
    for slot, p in want.items():
        assert abs(s[8 + slot] - p ** 0.6) <= 1e-12 * p ** 0.6, slot
    assert s[8 + 5:] == [0.0] * 3 and all(math.isinf(x) for x in m[8 + 5:])
    P.assert_trees_follow_from_their_leaves(s, m)
    # the next message takes the new maximum
    assert t.add(2, 1) == 0
    s, m, _ = t.read()
    assert abs(s[8 + 2] - prio(9.5) ** 0.6) <= 1e-12 * prio(9.5) ** 0.6
    P.assert_trees_follow_from_their_leaves(s, m)


def test_tree_entries_refuse_bad_sizes_and_launch_nothing(L):
    t = P.GpuTrees(37, 0.6)
    assert t.add(0, 37) == 0
    before = t.read()
    for kw in (dict(first=60, count=5), dict(first=-1, count=2), dict(first=0, count=0), dict(first=0, count=4, cap2=48)):
        assert t.add(**kw) != 0 and "xt_per_add" in L.load().xt_last_error().decode()
    assert t.update([1, 2], np.float32([1, 2]), 0.0) != 0                  # eps must be positive
    assert t.update([1] * 1025, np.float32([1] * 1025), EPS) != 0 and "1024" in L.load().xt_last_error().decode()
    assert t.read() == before
    for n, u, kw in ((1, [0.5], {}), (38 + 64, [0.5], {}), (37, [0.5] * 1025, {}), (37, [0.5], dict(b=0))):
        rc, slots, w = t.sample(n, u, 0.4, **kw)
        assert rc != 0 and (slots == -1).all() and np.isnan(w).all()
    rc, _, _ = t.sample(1, [0.5], 0.4)
    assert "cannot be sampled" in L.load().xt_last_error().decode()
    # a slot outside the tree is not stored through
    assert t.update([5, 64, -1], np.float32([2.0, 3.0, 4.0]), EPS) == 0
    s, m, _ = t.read()
    assert s[64:64 + 5] == before[0][64:64 + 5] and s[64 + 6:] == before[0][64 + 6:] and s[64 + 5] != before[0][64 + 5]
    P.assert_trees_follow_from_their_leaves(s, m)


# ------------------------------------------------------------------------------------------------ sampling
@pytest.mark.parametrize("name", NAMES)
def test_sample_on_the_device_trees_equals_the_restatement(cases, replayed, name):
    c = cases[name]
    t, (s, m, _) = replayed(name)
    rc, slots, w = t.sample(c.n, c.u, c.beta)
    assert rc == 0
    _, ref_slots, ref_w = P.sample(s, m, c.n, c.u, c.beta)
    assert slots.tolist() == ref_slots                                     # exactly, the u = 0 and u = 1 - 2^-53 rows included
    err = P.rel_err(w, ref_w)
    print("per sample", name, "weights rel", err, "| equal to the recorded indices:", slots.tolist() == c.idx)
    assert err <= 1e-12
    assert 0 <= slots.min() and slots.max() < c.n
    assert (c.n < c.capacity) == (name == "c707")                          # N < capacity and N = capacity are both here
    if name == "c64_edge":
        assert [c.u[i] for i in (0, 1, 2, -1)] == [0.0, 1.0 - 2.0 ** -53, 0.0, 1.0 - 2.0 ** -53]
        assert slots[0] == 0 and slots[2] == ref_slots[2]


def test_the_last_stored_slot_is_never_drawn_while_its_neighbours_are(cases, replayed):
    c = cases["c5"]
    t, _ = replayed("c5")
    rc, slots, _ = t.sample(c.n, c.u, c.beta)
    assert rc == 0 and set(slots.tolist()) == {0, 1, 2, 3}                 # 32 draws over 5 stored: slot 4 never
    c = cases["c707"]
    t, _ = replayed("c707")
    # 1024 strata: the first one from its start, every other one 0.999 of the way through -- the last stratum ends in
    # leaf N - 2 (its mass, at least (1e-3) ** 0.6, is more than a thousandth of a stratum), never in leaf N - 1
    rc, slots, _ = t.sample(c.n, [0.0] + [0.999] * 1023, c.beta)
    assert rc == 0 and slots[0] == 0 and slots[-1] == c.n - 2 and slots.max() == c.n - 2
    assert (np.diff(slots) >= 0).all()


# ------------------------------------------------------------------------------------------------ xt_dqn_loss_w
def _loss_inputs(b, a, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    d = dict(logits=f(b, a), value=f(b), t_logits=f(b, a) * 2, t_value=f(b), o_logits=f(b, a) * 2, o_value=f(b),
             action=rng.integers(0, a, b).astype(np.int32), reward=rng.standard_normal(b))
    d["done"] = (np.arange(b) % 3 == 0).astype(np.uint8)
    d["w"] = rng.uniform(0.05, 1.0, b)
    return d


def _heads(d, double):
    return (d["logits"], d["value"], d["t_logits"], d["t_value"], d["o_logits"] if double else None,
            d["o_value"] if double else None, d["action"], d["reward"], d["done"], GAMMA)


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("dueling", [False, True])
@pytest.mark.parametrize("b,a", [(5, 2), (32, 4), (33, 18)])
def test_dqn_loss_w_without_weights_is_xt_dqn_loss_bit_for_bit(L, b, a, dueling, double):
    d = _loss_inputs(b, a, 7 * b + a)
    rc0, plain = H.gpu_dqn_loss(*_heads(d, double), dueling)
    rc1, got = H.gpu_dqn_loss(*_heads(d, double), dueling, entry="xt_dqn_loss_w")
    assert rc0 == 0 and rc1 == 0
    for k, v in got.items():
        assert v.tobytes() == plain[k].tobytes(), k                        # (out[3] is never written: NaN bits on both sides)


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("dueling", [False, True])
@pytest.mark.parametrize("a", [2, 4, 18])
@pytest.mark.parametrize("b", [5, 32])
def test_dqn_loss_w_against_float64(L, b, a, dueling, double):
    d = _loss_inputs(b, a, 100 * b + a + 2 * dueling + double)
    rc, got = H.gpu_dqn_loss(*_heads(d, double), dueling, entry="xt_dqn_loss_w", weights=d["w"])
    assert rc == 0
    f64 = lambda x: None if x is None else np.asarray(x, np.float64)
    heads = [f64(x) for x in _heads(d, double)[:6]]
    ref = H.dqn_loss_ref(*heads, d["action"], d["reward"], d["done"], GAMMA, dueling, d["w"])
    plain = H.dqn_loss_ref(*heads, d["action"], d["reward"], d["done"], GAMMA, dueling)
    out = got["out"]
    print("dqn_loss_w: loss", out[0], ref["loss"], "| dlogits", H.rel_max(got["dlogits"], ref["dlogits"]))
    assert abs(ref["loss"] - plain["loss"]) > 1e-2 * abs(plain["loss"])    # the weights matter
    assert abs(out[0] - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"]))
    assert abs(out[1] - plain["abs_td"]) <= 1e-5 * max(1.0, plain["abs_td"])              # unweighted
    assert abs(out[2] - plain["mean_maxq"]) <= 1e-5 * max(1.0, abs(plain["mean_maxq"]))   # unweighted
    assert H.rel_max(got["dlogits"], ref["dlogits"]) <= 1e-5
    if dueling:
        assert H.rel_max(got["dvalue"], ref["dvalue"]) <= 1e-5
    else:
        assert not got["dvalue"].any()
    assert np.array_equal(got["astar"], ref["astar"])
    assert H.rel_max(out[4::2][:b], ref["delta"]) <= 1e-5                  # the terms the priority update reads


# ------------------------------------------------------------------------------------------------ xt_net_dqn_step_per
def _spec_pair(kind, a_dim, dueling):
    from xingtian_amd.model import netspec
    if kind == "cnn":
        return netspec.dqn_cnn((84, 84, 4), a_dim, dueling), H.oracle_spec("cnn", (84, 84, 4), a_dim)
    return netspec.dqn_mlp((4,), a_dim, 32, 1, dueling), H.oracle_spec("mlp", (4,), a_dim, 32, 1)


def _states(kind, rng, n):
    if kind == "cnn":
        return rng.integers(0, 256, (n, 84, 84, 4), dtype=np.uint8)
    return rng.standard_normal((n, 4)).astype(np.float32)


def _assert_step(got_loss, grads, ref, spec, ospec):
    assert abs(got_loss - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"])), (got_loss, ref["loss"])
    worst = 0.0
    for h, o in H.name_map(spec, ospec).items():
        r = ref["grads"][o]
        err = np.linalg.norm(grads[h].reshape(r.shape) - r) / (np.linalg.norm(r) + 1e-30)
        worst = max(worst, err)
        assert err <= 1e-5, (h, err)
    print("dqn per step: loss", got_loss, float(ref["loss"]), "| worst gradient tensor", worst)


def _primed_trees(cap, size, alpha, rng):
    """trees of a ring of ``cap`` rows with ``size`` stored transitions of distinct priorities"""
    t = P.GpuTrees(cap, alpha)
    assert t.add(0, size) == 0
    assert t.update(list(range(size)), rng.uniform(0.01, 3.0, size).astype(np.float32), EPS) == 0
    return t


@pytest.mark.parametrize("kind,b,dueling,double", [("mlp", b, du, do) for b in (5, 32) for du in (False, True)
                                                   for do in (False, True)] + [("cnn", 5, True, False), ("cnn", 32, True, False)])
def test_net_dqn_step_per_against_float64(L, kind, b, dueling, double):
    from xingtian_amd.model.hip_net import HipActorCritic
    a_dim = 2 if kind == "mlp" else 4
    alpha, beta = 0.6, 0.4
    spec, ospec = _spec_pair(kind, a_dim, dueling)
    rng = np.random.default_rng(b + 2 * dueling + double)
    p_on, p_tg = H.seeded_params(ospec, 1, dueling), H.seeded_params(ospec, 2, dueling)
    net, target = HipActorCritic(spec, max_batch=32, seed=0), HipActorCritic(spec, max_batch=32, seed=0)
    net.set_weights(H.to_keras_names(spec, ospec, p_on))
    target.set_weights(H.to_keras_names(spec, ospec, p_tg))
    target_before = target.params.clone()
    cap = 40
    size = 40 if b == 32 else 33                                           # a full ring, and one that is not
    cur, nxt = _states(kind, rng, cap), _states(kind, rng, cap)
    # rewards around +2, so that the TD errors share a sign: the 1-wide head's bias gradient is the scalar sum_b g_b, and
    # where the g_b cancel (sum |g_b| / |sum g_b| was 600 with centred rewards) its relative error measures the
    # cancellation -- 600 x 2^-24 = 3.6e-5 for ANY float32 head -- not the kernel; the bound stays the project's 1e-5
    action, reward = rng.integers(0, a_dim, cap).astype(np.int32), rng.standard_normal(cap) + 2.0
    done = (rng.random(cap) < 0.3).astype(np.uint8)
    t = _primed_trees(cap, size, alpha, rng)
    s0, m0, max0 = t.read()
    u = rng.random(b)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    terms = torch.full((2 * b,), float("nan"), dtype=torch.float32, device="cuda")
    per = dict(size=size, u=up(u), sum_tree=t.sum, min_tree=t.min, max_prio=t.max_prio, alpha=alpha, beta=beta, eps=EPS,
               terms_out=terms)
    out = net.dqn_step(target, net.to_device_obs(cur), net.to_device_obs(nxt), None, up(action), up(reward), up(done),
                       GAMMA, dueling, double, per=per)
    torch.cuda.synchronize()
    # the draw: the restatement on the tree as it was before the step
    _, ref_slots, ref_w = P.sample(s0, m0, size, u.tolist(), beta)
    slots, w = net.per_slots[:b].cpu().numpy(), net.per_weights[:b].cpu().numpy()
    assert slots.tolist() == ref_slots and P.rel_err(w, ref_w) <= 1e-12
    # loss and gradient on those slots with those weights
    orc = H.DqnOracle(ospec, p_on, p_tg, dueling, double, GAMMA, lr=3e-4, dtype=np.float64)
    ref = orc.step(cur[slots], nxt[slots], action[slots], reward[slots], done[slots], w, apply=False)
    _assert_step(float(out.cpu().numpy()[0]), net.grads_dict(), ref, spec, ospec)
    delta = terms.cpu().numpy()[0::2]
    assert H.rel_max(delta, ref["delta"]) <= 1e-5
    # the write-back: the sampled leaves take (|delta| + eps) ** alpha of the device's own terms, the last occurrence
    # of a slot wins, every other leaf is untouched, the ancestors follow
    s1, m1, max1 = t.read()
    prio = [float(abs(d)) + EPS for d in delta]
    assert max1 == max([max0] + prio)
    want = {int(sl): p for sl, p in zip(slots, prio)}
    for slot in range(cap):
        if slot in want:
            p = want[slot] ** alpha
            assert abs(s1[t.cap2 + slot] - p) <= 1e-12 * p and m1[t.cap2 + slot] == s1[t.cap2 + slot], slot
        else:
            assert s1[t.cap2 + slot] == s0[t.cap2 + slot] and m1[t.cap2 + slot] == m0[t.cap2 + slot], slot
    P.assert_trees_follow_from_their_leaves(s1, m1)
    assert torch.equal(target.params, target_before) and not bool(target.grads.any())     # the target net is forward only


def test_net_dqn_step_per_refusals_are_the_uniform_step_s(L):
    from xingtian_amd.model import netspec
    from xingtian_amd.model.hip_net import HipActorCritic
    spec = netspec.dqn_mlp((4,), 2, 32, 1, False)
    net, target = HipActorCritic(spec, max_batch=8, seed=0), HipActorCritic(spec, max_batch=8, seed=0)
    other = HipActorCritic(netspec.dqn_mlp((4,), 3, 32, 1, False), max_batch=8, seed=0)
    ring = torch.zeros((10, 4), dtype=torch.float32, device="cuda")
    lab = (torch.zeros(10, dtype=torch.int32, device="cuda"), torch.zeros(10, dtype=torch.float64, device="cuda"),
           torch.zeros(10, dtype=torch.uint8, device="cuda"))
    t = _primed_trees(10, 10, 0.6, np.random.default_rng(0))
    before = t.read()
    u = torch.full((4,), 0.5, dtype=torch.float64, device="cuda")
    step = lambda tgt, rg, uu, size=10: net.dqn_step(tgt, rg, rg, None, *lab, GAMMA, False, False, per=dict(
        size=size, u=uu, sum_tree=t.sum, min_tree=t.min, max_prio=t.max_prio, alpha=0.6, beta=0.4, eps=EPS))
    for tgt, rg, uu, word in ((net, ring, u, "own parameter buffers"), (other, ring, u, "same description"),
                              (target, ring, torch.full((9,), 0.5, dtype=torch.float64, device="cuda"), "batch"),
                              (target, torch.zeros((10, 8), dtype=torch.float32, device="cuda"), u, "row_bytes")):
        with pytest.raises(RuntimeError) as info:
            step(tgt, rg, uu)
        assert word in str(info.value) and "xt_net_dqn_step_per" in str(info.value), (word, str(info.value))
    with pytest.raises(RuntimeError) as info:
        step(target, ring, u, size=1)
    assert "cannot be sampled" in str(info.value)
    with pytest.raises(RuntimeError) as info:
        step(target, ring, u, size=11)
    assert "size" in str(info.value)
    net.set_dp(0, 2)
    with pytest.raises(RuntimeError) as info:
        step(target, ring, u)
    assert "data parallelism" in str(info.value)
    assert t.read() == before                                              # no refusal touched the trees


# ------------------------------------------------------------------------------------------------ alg_builder("DQN")
def _messages(kind, rng, a_dim, n_msg=3, rows=20):
    msgs = []
    for _ in range(n_msg):
        msgs.append({"cur_state": _states(kind, rng, rows), "next_state": _states(kind, rng, rows),
                     "action": rng.integers(0, a_dim, rows).astype(np.int32),
                     "reward": [float(x) for x in rng.standard_normal(rows)],
                     "done": [bool(x) for x in rng.random(rows) < 0.3]})
    return msgs


def _build(kind, a_dim, dueling, double, batch, buffer_size=50, freq=3, **per):
    from xingtian_amd.algorithm import alg_builder
    mc = {"dueling": dueling, "SEED": 3, "LR": 3e-4}
    if kind == "mlp":
        mc.update(HIDDEN_SIZE=32, NUM_LAYERS=1)
    info = {"actor": {"model_name": "DqnCnn" if kind == "cnn" else "DqnMlp", "type": "learner",
                      "state_dim": [84, 84, 4] if kind == "cnn" else [4], "action_dim": a_dim, "model_config": mc}}
    cfg = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1, "BUFFER_SIZE": buffer_size,
           "BATCH_SIZE": batch, "TARGET_UPDATE_FREQ": freq, "GAMMA": GAMMA, "double_dqn": double}
    cfg.update(per)
    return alg_builder("DQN", info, cfg)


@pytest.mark.parametrize("kind,dueling,double,batch", [("mlp", True, True, 32), ("cnn", False, False, 8)])
def test_dqn_algorithm_with_prioritized_replay_three_trains(L, kind, dueling, double, batch):
    from xingtian_amd.algorithm.dqn.dqn import PrioritizedDeviceReplay
    a_dim = 2 if kind == "mlp" else 4
    alg = _build(kind, a_dim, dueling, double, batch, prioritized_replay=True, prioritized_replay_beta_iters=4)
    buf = alg.buff
    assert alg.device_step and alg.prioritized and type(buf) is PrioritizedDeviceReplay and buf.sum_tree is None
    rng = np.random.default_rng(17)
    for m in _messages(kind, rng, a_dim):
        alg.prepare_data(m)
    assert buf.size() == 50 and buf.head == 10 and buf.cap2 == 64          # 60 rows into 50 slots: wrapped
    row_bytes = buf.cur_state[0].numel() * buf.cur_state.element_size()
    assert buf.bytes == 50 * (2 * row_bytes + 13) + 2 * 2 * 64 * 8
    read = lambda: (buf.sum_tree.cpu().tolist(), buf.min_tree.cpu().tolist())
    s, m = read()
    assert s[64:64 + 50] == [1.0] * 50 and s[64 + 50:] == [0.0] * 14 and float(buf.max_prio.item()) == 1.0
    P.assert_trees_follow_from_their_leaves(s, m)
    target_init = alg.target_actor.net.params.clone()
    random.seed(23)
    for t in range(3):
        beta = 0.4 + (t / 4.0) * (1.0 - 0.4)
        assert alg.per_beta() == beta                                      # linear from beta0 to 1.0 over 4 trains
        s, m = read()
        state = random.getstate()
        loss = alg.train()
        after = random.getstate()
        random.setstate(state)
        u = [random.random() for _ in range(batch)]                        # the same stream: what the train drew
        assert random.getstate() == after and isinstance(loss, float) and math.isfinite(loss)
        _, ref_slots, ref_w = P.sample(s, m, 50, u, beta)
        assert alg.actor.net.per_slots[:batch].cpu().tolist() == ref_slots
        assert P.rel_err(alg.actor.net.per_weights[:batch].cpu().numpy(), ref_w) <= 1e-12
        s1, m1 = read()
        assert s1 != s and float(buf.max_prio.item()) >= 1.0
        changed = {i for i in range(50) if s1[64 + i] != s[64 + i]}
        assert changed and changed <= set(ref_slots)                       # only sampled leaves moved
        P.assert_trees_follow_from_their_leaves(s1, m1)
        tp = alg.target_actor.net.params
        assert torch.equal(tp, target_init) if t < 2 else torch.equal(tp, alg.actor.net.params)
    assert alg.train_count == 3 and alg.actor.iterations == 3
    # a later message takes the running maximum priority
    alg.prepare_data(_messages(kind, rng, a_dim, n_msg=1, rows=3)[0])
    s, m = read()
    top = float(buf.max_prio.item()) ** 0.6
    assert all(abs(s[64 + i] - top) <= 1e-12 * top for i in (10, 11, 12)) and buf.head == 13
    P.assert_trees_follow_from_their_leaves(s, m)


def test_prioritized_train_on_one_stored_transition_raises_value_error(L):
    alg = _build("mlp", 2, False, False, 32, prioritized_replay=True)
    alg.prepare_data(_messages("mlp", np.random.default_rng(1), 2, n_msg=1, rows=1)[0])
    assert alg.buff.size() == 1
    with pytest.raises(ValueError) as info:
        alg.train()
    assert "at least 2" in str(info.value) and alg.train_count == 0
    alg.prepare_data(_messages("mlp", np.random.default_rng(2), 2, n_msg=1, rows=1)[0])
    assert math.isfinite(alg.train()) and alg.train_count == 1             # two stored: B = 2, both draws land on slot 0
    assert alg.actor.net.per_slots[:2].cpu().tolist() == [0, 0]
