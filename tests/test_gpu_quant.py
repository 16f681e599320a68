"""GPU tests of the quantile-regression (QR-DQN) path: the head ``xt_dqn_loss_quant`` alone against the float64
restatement (bars: four times the float32 NumPy restatement's own deviation, ``quant_helpers.head_bars``), the refusals of
the three entries, ``xt_net_dqn_step_quant`` against the float64 checker (uniform, double DQN, prioritised, n-step, both;
on the wide-head kernels and on the generic ones) at the project's standing bars (loss 1e-4, every gradient tensor 1e-5
by ``rel_max``), and ``alg_builder("DQN")`` with ``model_config.quantiles``."""
import numpy as np
import pytest
import torch

import dqn_helpers as H
import nstep_helpers as N
import per_helpers as P
import quant_helpers as Q

pytestmark = pytest.mark.gpu

GAMMA = Q.GAMMA
EPS = 1e-6
CAP = Q.CAP


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


# ------------------------------------------------------------------------------------------------ the head alone
@pytest.mark.parametrize("through_slots", [False, True])
@pytest.mark.parametrize("with_disc", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("shape", Q.HEAD_SHAPES, ids=["B%d_A%d_N%d" % s for s in Q.HEAD_SHAPES])
def test_dqn_loss_quant_against_float64(L, shape, double, weighted, with_disc, through_slots):
    b, a, n = shape
    c = Q.head_case(shape, double, weighted, with_disc, through_slots)
    ref = Q.head_ref(c)
    pl = c["planted"]
    gap = Q.argmax_gap(ref, pl)
    assert gap >= Q.ARGMAX_GAP, gap                           # the condition under which a* is comparable at all
    rc, got = Q.gpu_dqn_loss_quant(c)
    assert rc == 0
    measured, bars = Q.head_bars()
    terms = got["out"][4:4 + 2 * b].reshape(b, 2)
    errs = {"loss_b": H.rel_max(terms[:, 0], ref["loss_b"]), "dlogits": H.rel_max(got["dlogits"], ref["dlogits"]),
            "qstar": H.rel_max(got["maxq"], ref["qstar"]), "out": H.rel_max(got["out"][:3], Q.out_of(ref))}
    print("quant head", shape, (double, weighted, with_disc, through_slots), "errs", errs, "bars", bars)
    assert np.array_equal(got["astar"], ref["astar"])
    if "tie" in pl and a > 1:
        assert got["astar"][pl["tie"]] == 0                   # identical picking quantiles: the first index wins
    for k, e in errs.items():
        assert e <= bars[k], (k, e, bars[k])
    assert np.array_equal(terms[:, 1], got["maxq"])
    assert np.isnan(got["out"][3]) and np.isnan(got["out"][4 + 2 * b:]).all()       # nothing written past the terms
    # every column outside the taken action's quantiles, and dvalue: exactly 0 (written by the kernel over the NaN sentinels)
    taken = np.zeros((b, a, n), bool)
    taken[np.arange(b), ref["act"]] = True                    # (actions -1 and A are clamped into [0, A))
    dl = got["dlogits"].reshape(b, a, n)
    assert not np.isnan(dl).any() and (dl[~taken] == 0).all() and (got["dvalue"] == 0).all()
    if "zero" in pl:                                          # u_ij = 0 for every j: that quantile's gradient is exactly 0
        assert dl[pl["zero"], ref["act"][pl["zero"]], n // 2] == 0.0
    # the means: the kernel's own terms reduced in float64, to float32 rounding
    w = np.ones(b) if c["weights"] is None else c["weights"].astype(np.float32).astype(np.float64)
    t64 = terms.astype(np.float64)
    want = np.array([(w * t64[:, 0]).sum() / b, t64[:, 0].mean(), t64[:, 1].mean()])
    assert np.abs(got["out"][:3] - want).max() <= 2.0 ** -23 * max(1.0, np.abs(want).max())


def test_dqn_loss_quant_refusals_leave_the_outputs_untouched(L):
    c = Q.head_case((7, 2, 32), True, True, True, True)
    for kw in (dict(n=1), dict(n=257), dict(n=0), dict(a=0), dict(a=65), dict(kappa=0.0), dict(kappa=-1.0),
               dict(kappa=float("nan")), dict(kappa=float("inf")), dict(b=0), dict(misalign_out=True)):
        rc, got = Q.gpu_dqn_loss_quant(c, **kw)
        assert rc != 0, kw
        assert all(np.isnan(got[k]).all() for k in ("dlogits", "dvalue", "out", "maxq")) and (got["astar"] == -1).all(), kw


# ------------------------------------------------------------------------------------------------ networks and replay
def _nets(s, max_batch=32, mark=True, kappa=Q.KAPPA):
    from xingtian_amd.model.hip_net import HipActorCritic
    spec, ospec = s["spec"], s["ospec"]
    net, target = HipActorCritic(spec, max_batch=max_batch, seed=0), HipActorCritic(spec, max_batch=max_batch, seed=0)
    net.set_weights(H.to_keras_names(spec, ospec, s["p_on"]))
    target.set_weights(H.to_keras_names(spec, ospec, s["p_tg"]))
    if mark:
        net.set_quant(spec.quantiles, kappa)
        target.set_quant(spec.quantiles, kappa)
    return net, target


def _filled_replay(kind, net, a_dim, n_step):
    from xingtian_amd.algorithm.dqn.dqn import DeviceReplay
    ring = DeviceReplay(CAP, net.device, net.to_device_obs, n_step=n_step)
    store, msgs = N.fill(ring, CAP, Q.RING_SEED, a_dim=a_dim, states=Q.state_fn(kind))
    cur = {s: msgs[m]["cur_state"][t] for s, (m, t) in enumerate(store.slot)}
    nxt = {s: msgs[m]["next_state"][t] for s, (m, t) in enumerate(store.slot)}
    return ring, store, cur, nxt


def _primed_trees(size, alpha, rng, ok):
    """trees whose leaves of the slots in ``ok`` hold priorities in [0.01, 3] and the others eps: a draw of 32 then stays
    among ``ok`` with probability 0.999"""
    t = P.GpuTrees(CAP, alpha)
    assert t.add(0, size) == 0
    delta = np.zeros(size, np.float32)
    delta[ok] = rng.uniform(0.01, 3.0, len(ok))
    assert t.update(list(range(size)), delta, EPS) == 0
    return t


# ------------------------------------------------------------------------------------------------ the whole step
_REFS = {}


def _step_ref(case, s, states, nstates, act, rew, disc, done, w):
    """the float64 oracle's step on one case's minibatch, computed once and shared by the wide and the generic arm"""
    if case not in _REFS:
        kind, a, n, _ = case
        orc = Q.QuantOracle(s["ospec"], s["p_on"], s["p_tg"], a, n, Q.KAPPA, s["double"], 3e-4)
        _REFS[case] = (orc.step(states, nstates, act, rew, disc, done, w), states, act, w)
    ref, states0, act0, w0 = _REFS[case]
    assert np.array_equal(states0, states) and np.array_equal(act0, act)               # the same minibatch in both arms
    assert (w is None and w0 is None) or np.array_equal(w0, w)
    return ref


@pytest.mark.parametrize("wide", [True, False], ids=["wide", "generic"])
@pytest.mark.parametrize("case", Q.STEP_CASES, ids=["%s_A%d_N%d_%s" % c for c in Q.STEP_CASES])
def test_net_dqn_step_quant_against_float64(L, case, wide):
    from xingtian_amd.algorithm.dqn.dqn import nstep_targets
    kind, a_dim, n, variant = case
    s = Q.step_setup(*case)
    prioritised, n_step, double = s["prioritised"], s["n_step"], s["double"]
    b, alpha, beta = Q.BATCH, 0.6, 0.4
    spec, ospec, ok = s["spec"], s["ospec"], s["ok"]
    assert len(ok) >= b
    net, target = _nets(s)
    net.set_dist_wide(wide)
    target.set_dist_wide(wide)
    target_before = target.params.clone()
    ring, store, cur, nxt = _filled_replay(kind, net, a_dim, n_step)
    rng = np.random.default_rng(len(variant) + 7 * (kind == "cnn") + n)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if n_step > 1:
        labels = lambda sl: nstep_targets(sl, *N.host_rings(ring), GAMMA, n_step, CAP)
    else:
        h = lambda x: x.cpu().numpy()
        labels = lambda sl: (np.asarray(sl, np.int32), h(ring.action)[sl], h(ring.reward)[sl], np.full(len(sl), GAMMA),
                             h(ring.done)[sl])
    # the device rings hold what the host-side table was counted on
    for got, want in zip(labels(np.arange(CAP)), Q.host_labels(kind, a_dim, n_step)(np.arange(CAP))):
        assert np.array_equal(got, want)
    kw = dict(follow=ring.follow, n=n_step, quant=True) if n_step > 1 else dict(quant=True)
    args = (ring.action, ring.reward, ring.done, GAMMA, False, double)
    if prioritised:
        t = _primed_trees(CAP, alpha, rng, ok)
        s0, m0, max0 = t.read()
        for _ in range(100):
            u = rng.random(b)
            if set(P.sample(s0, m0, CAP, u.tolist(), beta)[1]) <= set(ok.tolist()):
                break
        else:
            raise AssertionError("no well-conditioned prioritised draw")
        terms = torch.full((2 * b,), float("nan"), dtype=torch.float32, device="cuda")
        per = dict(size=CAP, u=up(u), sum_tree=t.sum, min_tree=t.min, max_prio=t.max_prio, alpha=alpha, beta=beta, eps=EPS,
                   terms_out=terms)
        out = net.dqn_step(target, ring.cur_state, ring.next_state, None, *args, per=per, **kw)
        torch.cuda.synchronize()
        _, ref_slots, ref_w = P.sample(s0, m0, CAP, u.tolist(), beta)
        slots, w = net.per_slots[:b].cpu().numpy(), net.per_weights[:b].cpu().numpy()
        assert slots.tolist() == ref_slots and P.rel_err(w, ref_w) <= 1e-12
    else:
        slots, w = rng.permutation(ok)[:b], None
        out = net.dqn_step(target, ring.cur_state, ring.next_state, up(slots), *args, **kw)
        torch.cuda.synchronize()
    boot, act, rew, disc, done = labels(slots)
    if n_step > 1:                                            # the five labels the gather left: the host's, bit for bit
        for name, want in (("boot", boot), ("action", act), ("reward", rew), ("disc", disc), ("done", done)):
            got = getattr(net, "nstep_" + name)[:b].cpu().numpy()
            assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), name
        assert (boot != slots).any() and len(set(disc.tolist())) > 1
    ref = _step_ref(case, s, np.stack([cur[x] for x in slots]), np.stack([nxt[j] for j in boot]), act, rew, disc, done, w)
    gap = Q.argmax_gap(ref, {})
    assert gap >= Q.ARGMAX_GAP, gap
    got = out.cpu().numpy()
    Q.assert_step(float(got[0]), net.grads_dict(), ref, spec, ospec, "%s %s %s" % (kind, variant, "wide" if wide else "generic"))
    assert abs(got[1] - ref["mean_loss"]) <= 1e-4 * max(1.0, ref["mean_loss"])
    assert abs(got[2] - ref["mean_q"]) <= 1e-4 * max(1.0, np.abs(ref["pick"]).max())
    assert torch.equal(target.params, target_before) and not bool(target.grads.any())     # the target net is forward only
    if not prioritised:
        return
    # the leaves of the start slots take (loss_b + eps) ** alpha, formed on the host from the kernel's own terms
    loss_b = terms.cpu().numpy()[0::2]
    assert H.rel_max(loss_b, ref["loss_b"]) <= 1e-4 and (loss_b >= 0).all()
    s1, m1, max1 = t.read()
    prio = [float(abs(d)) + EPS for d in loss_b]
    assert max1 == max([max0] + prio)
    want = {int(sl): p for sl, p in zip(slots, prio)}         # (the last occurrence of a slot wins)
    for slot in range(CAP):
        if slot in want:
            p = want[slot] ** alpha
            assert abs(s1[t.cap2 + slot] - p) <= 1e-12 * p and m1[t.cap2 + slot] == s1[t.cap2 + slot], slot
        else:
            assert s1[t.cap2 + slot] == s0[t.cap2 + slot] and m1[t.cap2 + slot] == m0[t.cap2 + slot], slot
    P.assert_trees_follow_from_their_leaves(s1, m1)


def test_step_entries_refuse_the_wrong_mark_and_name_the_right_entry(L):
    s = Q.step_setup("mlp", 2, 8, "plain")
    net, target = _nets(s, 8)
    ring, _, _, _ = _filled_replay("mlp", net, 2, 1)
    slots = torch.arange(4, dtype=torch.int32, device="cuda")
    args = (ring.cur_state, ring.next_state, slots, ring.action, ring.reward, ring.done, GAMMA)
    net.grads.zero_()
    # a quantile pair at the scalar entries (plain, n-step, prioritised) and at the C51 entry
    with pytest.raises(RuntimeError, match="xt_net_dqn_step: the net is marked quantile.*xt_net_dqn_step_quant"):
        net.dqn_step(target, *args, False, False)
    follow = torch.zeros(CAP, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="xt_net_dqn_step_n: the net is marked quantile.*xt_net_dqn_step_quant"):
        net.dqn_step(target, *args, False, False, follow=follow, n=2)
    with pytest.raises(RuntimeError, match="xt_net_dqn_step_dist: the net is marked quantile.*xt_net_dqn_step_quant"):
        net.dqn_step(target, *args, False, False, dist=True)
    # dueling
    with pytest.raises(RuntimeError, match="no dueling stream with a quantile head"):
        net.dqn_step(target, *args, True, False, quant=True)
    # mark mismatches between the two nets
    target.set_quant(8, 0.5)
    with pytest.raises(RuntimeError, match="same quantiles and kappa"):
        net.dqn_step(target, *args, False, False, quant=True)
    target.set_quant(4, Q.KAPPA)
    with pytest.raises(RuntimeError, match="same quantiles and kappa"):
        net.dqn_step(target, *args, False, False, quant=True)
    target.set_quant(1, 0.0)
    with pytest.raises(RuntimeError, match="same quantiles and kappa"):
        net.dqn_step(target, *args, False, False, quant=True)
    # a C51 net at the quantile entry, and both marks on one net
    target.set_dist(8, -10.0, 10.0)
    with pytest.raises(RuntimeError, match="xt_net_dqn_step_quant: the net is marked distributional.*xt_net_dqn_step_dist"):
        net.dqn_step(target, *args, False, False, quant=True)
    with pytest.raises(RuntimeError, match="xt_net_set_quant: the net is marked distributional"):
        target.set_quant(8, Q.KAPPA)
    assert target.dist == (8, -10.0, 10.0) and getattr(target, "quant", None) is None
    with pytest.raises(RuntimeError, match="xt_net_set_dist: the net is marked quantile"):
        net.set_dist(8, -10.0, 10.0)
    target.set_dist(1, 0.0, 0.0)
    # xt_net_set_quant's own refusals
    with pytest.raises(RuntimeError, match="no multiple of quantiles"):
        target.set_quant(5, Q.KAPPA)
    for bad in (0, 257, -2):
        with pytest.raises(RuntimeError, match="quantiles = .* outside \\[1, 256\\]"):
            target.set_quant(bad, Q.KAPPA)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match="kappa must be finite and > 0"):
            target.set_quant(8, bad)
    with pytest.raises(RuntimeError, match="not marked distributional"):
        target.set_dist_wide(True)
    torch.cuda.synchronize()
    assert not bool(net.grads.any())                          # nothing was launched
    target.set_quant(8, Q.KAPPA)
    target.set_dist_wide(False)                               # works on a quantile-marked net
    target.set_dist_wide(True)
    net.dqn_step(target, *args, False, False, quant=True)
    torch.cuda.synchronize()
    assert bool(net.grads.any())


def test_more_than_64_actions_are_refused_by_the_quantile_step(L):
    from xingtian_amd.model import netspec
    from xingtian_amd.model.hip_net import HipActorCritic
    spec = netspec.dqn_mlp((4,), 65, 32, 1, False, 1, 2)
    net, target = HipActorCritic(spec, max_batch=8, seed=0), HipActorCritic(spec, max_batch=8, seed=1)
    net.set_quant(2, Q.KAPPA)
    target.set_quant(2, Q.KAPPA)
    ring, _, _, _ = _filled_replay("mlp", net, 2, 1)
    slots = torch.arange(4, dtype=torch.int32, device="cuda")
    net.grads.zero_()
    with pytest.raises(RuntimeError, match="A = 65 exceeds 64"):
        net.dqn_step(target, ring.cur_state, ring.next_state, slots, ring.action, ring.reward, ring.done, GAMMA, False, False,
                     quant=True)
    torch.cuda.synchronize()
    assert not bool(net.grads.any())


# ------------------------------------------------------------------------------------------------ through the plugin pair
def test_dqn_algorithm_with_quantiles_trains_predicts_and_round_trips_its_weights(L):
    from xingtian_amd.algorithm import alg_builder
    from xingtian_amd.algorithm.dqn.dqn import quant_q
    a_dim, n, batch = 2, 8, Q.BATCH
    mc = {"quantiles": n, "SEED": 3, "LR": 3e-4, "HIDDEN_SIZE": 32, "NUM_LAYERS": 1}
    info = {"actor": {"model_name": "DqnMlp", "type": "learner", "state_dim": [4], "action_dim": a_dim, "model_config": mc}}
    cfg = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1, "BUFFER_SIZE": CAP, "BATCH_SIZE": batch,
           "TARGET_UPDATE_FREQ": 2, "GAMMA": GAMMA, "double_dqn": False}
    alg = alg_builder("DQN", info, cfg)
    assert alg.device_step and alg.quantiles == n and alg.atoms == 1 and alg.actor.net.quant == (n, 1.0)
    s = Q.step_setup("mlp", a_dim, n, "plain")
    spec, ospec = s["spec"], s["ospec"]
    assert list(alg.actor.net.spec.names.items()) == list(spec.names.items())
    msgs, store = Q.ring_rows("mlp", a_dim)
    for m in msgs:
        alg.prepare_data(m)
    cur = {sl: msgs[m]["cur_state"][t] for sl, (m, t) in enumerate(store.slot)}
    nxt = {sl: msgs[m]["next_state"][t] for sl, (m, t) in enumerate(store.slot)}
    alg.actor.set_weights(H.to_keras_names(spec, ospec, s["p_on"]))
    alg.target_actor.set_weights(H.to_keras_names(spec, ospec, s["p_tg"]))
    net, buf = alg.actor.net, alg.buff
    net.lib = N.CountingLib(net.lib)
    copy = lambda p: {k: v.copy() for k, v in p.items()}
    orc = Q.QuantOracle(ospec, copy(s["p_on"]), copy(s["p_tg"]), a_dim, n, 1.0, False, 3e-4)
    slots = np.random.default_rng(17).permutation(s["ok"])[:batch]
    target_init = alg.target_actor.net.params.clone()
    h = lambda x: x.cpu().numpy()
    batch_args = (np.stack([cur[x] for x in slots]), np.stack([nxt[x] for x in slots]), h(buf.action)[slots],
                  h(buf.reward)[slots], np.full(batch, GAMMA), h(buf.done)[slots])
    losses = []
    for t in range(1, 4):                                     # the same replayed batch three times, a target sync after the second
        loss = alg.train_on_slots(slots.tolist())
        if t == 1:
            Q.assert_step(loss, net.grads_dict(), orc.step(*batch_args), spec, ospec, "plugin train 1")
        ref = orc.step(*batch_args, apply=True)
        print("quant train", t, "loss", loss, float(ref["loss"]))
        assert np.isfinite(loss) and abs(loss - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"])), (t, loss, ref["loss"])
        losses.append(loss)
        if t % 2 == 0:
            orc.sync_target()
        tp = alg.target_actor.net.params
        assert torch.equal(tp, target_init) if t < 2 else (torch.equal(tp, alg.actor.net.params) == (t == 2))
    assert losses[1] < losses[0]                              # (the third is taken against the synced target)
    assert alg.train_count == 3 and alg.actor.iterations == 3
    calls = net.lib.calls
    assert calls["xt_net_dqn_step_quant"] == 3 and calls["xt_net_dqn_step_dist"] == 0 and calls["xt_net_dqn_step"] == 0
    x = np.stack([cur[sl] for sl in range(9)])
    q = alg.actor.predict(x)
    logits = net.forward(x)[0].cpu().numpy()
    assert q.shape == (9, a_dim) and q.dtype == np.float32 and logits.shape == (9, a_dim * n)
    assert np.array_equal(q, quant_q(logits.reshape(9, a_dim, n)))
    want = orc.net.forward(x)[0].reshape(9, a_dim, n).mean(-1)
    assert np.abs(q - want).max() <= 1e-4 * max(1.0, np.abs(want).max())
    # the A * N wide head goes through get_weights / set_weights unchanged
    w = alg.actor.get_weights()
    head = spec.pi_name + "/kernel"
    assert w[head].shape == (32, a_dim * n) and w[spec.pi_name + "/bias"].shape == (a_dim * n,)
    alg.target_actor.set_weights(w)
    w2 = alg.target_actor.get_weights()
    assert sorted(w2) == sorted(w) and all(np.array_equal(w[k], w2[k]) for k in w)
    assert np.array_equal(alg.target_actor.predict(x), q)
