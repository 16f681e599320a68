"""GPU tests of n-step returns: ``xt_replay_gather_nstep`` against ``nstep_targets`` plus a NumPy gather (bit-exact), the
head with a per-sample discount (``xt_dqn_loss_n``) and ``xt_net_dqn_step_n`` against the float64 checker fed with the
host's n-step labels, the refusals, and ``alg_builder("DQN")`` with ``n_step``."""
import ctypes
import random

import numpy as np
import pytest
import torch

import dqn_helpers as H
import nstep_helpers as N
import per_helpers as P

pytestmark = pytest.mark.gpu

GAMMA = N.GAMMA
EPS = 1e-6
CAP = 50


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


def _bits(x):
    return x.contiguous().view(torch.uint8)


# ------------------------------------------------------------------------------------------------ xt_replay_gather_nstep
@pytest.fixture(scope="module")
def byte_rings(L):
    """row_bytes -> (DeviceReplay of capacity 50 filled with the CPU test's message table, its BruteStore)"""
    from xingtian_amd.algorithm.dqn.dqn import DeviceReplay
    made = {}

    def get(row_bytes):
        if row_bytes not in made:
            rows = lambda tags, nxt: np.random.default_rng(int(tags[0]) * 2 + nxt).integers(
                0, 256, (len(tags), row_bytes), dtype=np.uint8)
            ring = DeviceReplay(CAP, "cuda:0", n_step=3)
            store, _ = N.fill(ring, CAP, 11, states=rows)
            made[row_bytes] = (ring, store)
        return made[row_bytes]
    return get


@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("b", [1, 33])
@pytest.mark.parametrize("row_bytes", [16, 28224])
def test_gather_nstep_rows_and_labels_are_bit_exact(L, byte_rings, row_bytes, b, n):
    from xingtian_amd.algorithm.dqn.dqn import nstep_targets
    ring, store = byte_rings(row_bytes)
    assert store.evicted and ring.size() == CAP
    rng = np.random.default_rng(row_bytes + 10 * b + n)
    if b == 1:
        slots = [int(rng.integers(0, CAP))]
    else:
        slots = rng.permutation(CAP)[:b].tolist()
        slots[:5] = [CAP - 1, 0, CAP - 1, 7, CAP + 3]                          # unsorted, a duplicate, both ends, one outside
        causes = {store.target(s, n)["cause"] for s in slots if 0 <= s < CAP}
        assert n == 1 or causes >= set(N.CAUSES) - ({"done_mid"} if n == 2 else set())
    rc, dst, lab = N.gpu_gather_nstep(ring, slots, n)
    assert rc == 0
    want = nstep_targets(slots, *N.host_rings(ring), GAMMA, n, CAP)
    for k, w in zip(("boot", "action", "reward", "disc", "done"), want):
        assert np.array_equal(lab[k].cpu().numpy().view(np.uint8), w.view(np.uint8)), k       # bit for bit
    live = [s for s in slots if 0 <= s < CAP]
    brute, _ = store.targets(live, n)
    keep = np.asarray([0 <= s < CAP for s in slots])
    for got, w in zip(want, brute):
        assert np.array_equal(got[keep], w)
    nxt = ring.next_state.cpu().numpy()
    rows = np.stack([nxt[j] if 0 <= s < CAP else np.zeros(row_bytes, np.uint8) for s, j in zip(slots, want[0])])
    assert np.array_equal(dst.cpu().numpy(), rows)
    if n == 1:
        rc1, plain = H.gpu_replay_gather(ring.next_state, torch.tensor(slots, dtype=torch.int32, device="cuda"))
        assert rc1 == 0 and torch.equal(dst, plain)


def test_gather_nstep_refusals_launch_nothing(L, byte_rings):
    ring, _ = byte_rings(16)
    untouched = lambda dst, lab: bool((dst == 0xA5).all()) and bool((lab["boot"] == -7).all()) and \
        bool(torch.isnan(lab["reward"]).all()) and bool((lab["done"] == 0xA5).all())
    for kw, word in ((dict(n=0), "outside [1, 256]"), (dict(n=257), "outside [1, 256]"), (dict(n=3, follow=None), "null"),
                     (dict(n=3, labels=False), "null label"), (dict(n=3, b=0), "bad sizes")):
        rc, dst, lab = N.gpu_gather_nstep(ring, [1, 2, 3], **kw)
        assert rc != 0 and untouched(dst, lab), kw
        msg = L.load().xt_last_error().decode()
        assert "xt_replay_gather_nstep" in msg and word in msg, (kw, msg)
    rc, dst, lab = N.gpu_gather_nstep(ring, [1, 2, 3], 256)
    assert rc == 0 and not untouched(dst, lab)


# ------------------------------------------------------------------------------------------------ xt_dqn_loss_n
def _loss_inputs(b, a, seed):
    rng = np.random.default_rng(seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    d = dict(logits=f(b, a), value=f(b), t_logits=f(b, a) * 2, t_value=f(b), o_logits=f(b, a) * 2, o_value=f(b),
             action=rng.integers(0, a, b).astype(np.int32), reward=rng.standard_normal(b))
    d["done"] = (np.arange(b) % 3 == 2).astype(np.uint8)
    d["w"] = rng.uniform(0.05, 1.0, b)
    d["disc"] = GAMMA ** rng.integers(1, 6, b).astype(np.float64)
    if b > 1:
        d["disc"][:2] = [GAMMA, GAMMA ** 5]
    return d


def _heads(d, double):
    return (d["logits"], d["value"], d["t_logits"], d["t_value"], d["o_logits"] if double else None,
            d["o_value"] if double else None, d["action"], d["reward"], d["done"], GAMMA)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("dueling", [False, True])
@pytest.mark.parametrize("b,a", [(1, 2), (33, 18)])
def test_dqn_loss_n_against_float64_and_its_two_bit_twins(L, b, a, dueling, double, weighted):
    d = _loss_inputs(b, a, 100 * b + a + 2 * dueling + double)
    w = d["w"] if weighted else None
    rc, got = H.gpu_dqn_loss(*_heads(d, double), dueling, entry="xt_dqn_loss_n", weights=w, disc=d["disc"])
    assert rc == 0
    f64 = lambda x: None if x is None else np.asarray(x, np.float64)
    heads = [f64(x) for x in _heads(d, double)[:6]]
    ref = H.dqn_loss_ref(*heads, d["action"], d["reward"], d["done"], GAMMA, dueling, w, d["disc"])
    flat = H.dqn_loss_ref(*heads, d["action"], d["reward"], d["done"], GAMMA, dueling, w, np.full(b, GAMMA))
    out = got["out"]
    print("dqn_loss_n: loss", out[0], ref["loss"], "| dlogits", H.rel_max(got["dlogits"], ref["dlogits"]),
          "| maxq", H.rel_max(got["maxq"], ref["maxq"]))
    if b > 1:
        assert abs(ref["loss"] - flat["loss"]) > 1e-3 * abs(flat["loss"])  # the discounts matter
    assert np.array_equal(got["astar"], ref["astar"])
    boot = (d["reward"] + d["disc"] * got["maxq"].astype(np.float64)).astype(np.float32)
    assert np.array_equal(got["y"], np.where(d["done"].astype(bool), d["reward"].astype(np.float32), boot))   # from its own maxq
    assert abs(out[0] - ref["loss"]) <= 1e-4 * abs(ref["loss"])
    assert abs(out[1] - ref["abs_td"]) <= 1e-5 * max(1.0, ref["abs_td"])
    assert abs(out[2] - ref["mean_maxq"]) <= 1e-5 * max(1.0, abs(ref["mean_maxq"]))
    assert H.rel_max(got["maxq"], ref["maxq"]) <= 1e-5
    assert H.rel_max(got["dlogits"], ref["dlogits"]) <= 1e-5
    if dueling:
        assert H.rel_max(got["dvalue"], ref["dvalue"]) <= 1e-5
    else:
        assert not got["dvalue"].any()
    # disc == NULL is xt_dqn_loss_w; disc filled with gamma is the scalar-gamma call: bit for bit
    rc0, plain = H.gpu_dqn_loss(*_heads(d, double), dueling, entry="xt_dqn_loss_w", weights=w)
    rc1, null = H.gpu_dqn_loss(*_heads(d, double), dueling, entry="xt_dqn_loss_n", weights=w)
    rc2, filled = H.gpu_dqn_loss(*_heads(d, double), dueling, entry="xt_dqn_loss_n", weights=w, disc=np.full(b, GAMMA))
    assert rc0 == 0 and rc1 == 0 and rc2 == 0
    for k, v in plain.items():
        assert null[k].tobytes() == v.tobytes(), k                         # (out[3] is never written: NaN bits on both sides)
        assert filled[k].tobytes() == v.tobytes(), k


# ------------------------------------------------------------------------------------------------ xt_net_dqn_step_n
def _spec_pair(kind, a_dim, dueling):
    from xingtian_amd.model import netspec
    if kind == "cnn":
        return netspec.dqn_cnn((84, 84, 4), a_dim, dueling), H.oracle_spec("cnn", (84, 84, 4), a_dim)
    return netspec.dqn_mlp((4,), a_dim, 32, 1, dueling), H.oracle_spec("mlp", (4,), a_dim, 32, 1)


def _state_fn(kind):
    if kind == "cnn":
        return lambda tags, nxt: np.random.default_rng(int(tags[0]) * 2 + nxt).integers(
            0, 256, (len(tags), 84, 84, 4), dtype=np.uint8)
    return lambda tags, nxt: np.random.default_rng(int(tags[0]) * 2 + nxt).standard_normal((len(tags), 4)).astype(np.float32)


def _nets(spec, ospec, dueling, max_batch=32):
    from xingtian_amd.model.hip_net import HipActorCritic
    p_on, p_tg = H.seeded_params(ospec, 1, dueling), H.seeded_params(ospec, 2, dueling)
    net, target = HipActorCritic(spec, max_batch=max_batch, seed=0), HipActorCritic(spec, max_batch=max_batch, seed=0)
    net.set_weights(H.to_keras_names(spec, ospec, p_on))
    target.set_weights(H.to_keras_names(spec, ospec, p_tg))
    return net, target, p_on, p_tg


def _filled_replay(kind, net, a_dim, n_step=3):
    """-> (DeviceReplay [50] fed with the message table, store, all state rows and next-state rows by slot (host))"""
    from xingtian_amd.algorithm.dqn.dqn import DeviceReplay
    ring = DeviceReplay(CAP, net.device, net.to_device_obs, n_step=n_step)
    # rewards around +2, so that the TD errors share a sign (see test_net_dqn_step_per_against_float64: the 1-wide head's
    # bias gradient is sum_b g_b, and its relative error measures the cancellation among them, not the kernel)
    store, msgs = N.fill(ring, CAP, 11, a_dim=a_dim, states=_state_fn(kind), reward_shift=2.0)
    cur = {s: msgs[m]["cur_state"][t] for s, (m, t) in enumerate(store.slot)}
    nxt = {s: msgs[m]["next_state"][t] for s, (m, t) in enumerate(store.slot)}
    return ring, store, cur, nxt


MARGIN = 1e-6
_MARGINS = {}


def _kink_margins(kind, a_dim):
    """slot -> the smallest |pre-activation| of any ReLU unit in the float64 forward of the online net (seed 1) on that
    slot's state row.  A float32 sum of up to 3136 products of magnitude below 1 carries an absolute error of about
    sqrt(K) 2^-24 |partial sums| ~ 1e-7, so a unit whose float64 pre-activation is closer to zero than that may come out
    on the other side of the kink in ANY float32 implementation; its whole contribution to the gradient then differs,
    which no kernel accuracy can mend (one such unit among the 3136 of conv3 moves a 5-row gradient by 1e-4 and more).
    Among the 10^6 units of 50 random frames a few always lie that close (slot 22: 5.7e-9), so the tests below draw their
    minibatches among the rows whose units all keep MARGIN = 1e-6, ten times that error, from zero."""
    if kind not in _MARGINS:
        from oracle import nets
        ospec = H.oracle_spec(kind, (84, 84, 4) if kind == "cnn" else (4,), a_dim, 32, 1)
        msgs, store = N.make_messages(CAP, 11, a_dim=a_dim, states=_state_fn(kind)), N.BruteStore(CAP)
        for m in msgs:
            store.add(m)
        net = nets.ActorCritic(ospec, H.seeded_params(ospec, 1, True), np.float64)
        net.forward(np.stack([msgs[m]["cur_state"][t] for m, t in store.slot]))
        _MARGINS[kind] = np.min([np.abs(z.reshape(CAP, -1)).min(1) for _, _, z in net.cache[0]], axis=0)
    return _MARGINS[kind]


def _well_conditioned(kind, a_dim, draw):
    """the first minibatch ``draw()`` returns (-> slots, anything else) whose rows all keep MARGIN from the kink"""
    margins = _kink_margins(kind, a_dim)
    for _ in range(500):
        slots, rest = draw()
        if margins[np.asarray(slots)].min() >= MARGIN:
            return slots, rest
    raise AssertionError("no well-conditioned minibatch in 500 draws")


def _assert_step(got_loss, grads, ref, spec, ospec):
    worst = 0.0
    errs = {}
    for h, o in H.name_map(spec, ospec).items():
        r = ref["grads"][o]
        errs[h] = np.linalg.norm(grads[h].reshape(r.shape) - r) / (np.linalg.norm(r) + 1e-30)
        worst = max(worst, errs[h])
    print("dqn n-step: loss", got_loss, float(ref["loss"]), "| worst gradient tensor", worst)
    assert abs(got_loss - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"])), (got_loss, ref["loss"])
    for h, err in errs.items():
        assert err <= 1e-5, (h, err)


def _primed_trees(size, alpha, rng):
    t = P.GpuTrees(CAP, alpha)
    assert t.add(0, size) == 0
    assert t.update(list(range(size)), rng.uniform(0.01, 3.0, size).astype(np.float32), EPS) == 0
    return t


def _per_kw(t, u, alpha=0.6, beta=0.4, terms=None):
    return dict(size=CAP, u=u, sum_tree=t.sum, min_tree=t.min, max_prio=t.max_prio, alpha=alpha, beta=beta, eps=EPS,
                terms_out=terms)


@pytest.mark.parametrize("prioritised", [False, True])
@pytest.mark.parametrize("dueling,double", [(False, False), (True, True)])
@pytest.mark.parametrize("b", [5, 32])
@pytest.mark.parametrize("kind", ["mlp", "cnn"])
def test_net_dqn_step_n_against_float64(L, kind, b, dueling, double, prioritised):
    from xingtian_amd.algorithm.dqn.dqn import nstep_targets
    n, a_dim, alpha, beta = 3, (2 if kind == "mlp" else 4), 0.6, 0.4
    spec, ospec = _spec_pair(kind, a_dim, dueling)
    net, target, p_on, p_tg = _nets(spec, ospec, dueling)
    target_before = target.params.clone()
    ring, store, cur, nxt = _filled_replay(kind, net, a_dim)
    rng = np.random.default_rng(b + 2 * dueling + double)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    args = (ring.action, ring.reward, ring.done, GAMMA, dueling, double, ring.follow, n)
    if prioritised:
        t = _primed_trees(CAP, alpha, rng)
        s0, m0, max0 = t.read()

        def draw():
            u = rng.random(b)
            return P.sample(s0, m0, CAP, u.tolist(), beta)[1], u
        _, u = _well_conditioned(kind, a_dim, draw)
        terms = torch.full((2 * b,), float("nan"), dtype=torch.float32, device="cuda")
        out = net.dqn_step(target, ring.cur_state, ring.next_state, None, *args, per=_per_kw(t, up(u), alpha, beta, terms))
        torch.cuda.synchronize()
        _, ref_slots, ref_w = P.sample(s0, m0, CAP, u.tolist(), beta)
        slots, w = net.per_slots[:b].cpu().numpy(), net.per_weights[:b].cpu().numpy()
        assert slots.tolist() == ref_slots and P.rel_err(w, ref_w) <= 1e-12
    else:
        slots, w = _well_conditioned(kind, a_dim, lambda: (rng.permutation(CAP)[:b].astype(np.int32), None))
        out = net.dqn_step(target, ring.cur_state, ring.next_state, up(slots), *args)
        torch.cuda.synchronize()
    # the labels the gather left: the host's, bit for bit; the brute force agrees on boot slot, action and done
    boot, act_n, rew_n, disc_n, done_n = nstep_targets(slots, *N.host_rings(ring), GAMMA, n, CAP)
    for name, want in (("boot", boot), ("action", act_n), ("reward", rew_n), ("disc", disc_n), ("done", done_n)):
        got = getattr(net, "nstep_" + name)[:b].cpu().numpy()
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), name
    brute, rows = store.targets(slots.tolist(), n)
    for got, want in zip((boot, act_n, rew_n, disc_n, done_n), brute):
        assert np.array_equal(got, want)
    assert (boot != slots).any() and len(set(disc_n.tolist())) > 1
    # loss and gradient: the float64 oracle on the start rows, the boot rows and those labels
    orc = H.DqnOracle(ospec, p_on, p_tg, dueling, double, GAMMA, lr=3e-4, dtype=np.float64)
    ref = orc.step(np.stack([cur[s] for s in slots]), np.stack([nxt[j] for j in boot]), act_n, rew_n, done_n, w, disc_n,
                   apply=False)
    _assert_step(float(out.cpu().numpy()[0]), net.grads_dict(), ref, spec, ospec)
    assert torch.equal(target.params, target_before) and not bool(target.grads.any())     # the target net is forward only
    if not prioritised:
        return
    # the write-back goes to the START slots, each at its index (the last occurrence of a slot wins); every other leaf
    # is untouched, the boot slots' included
    delta = terms.cpu().numpy()[0::2]
    assert H.rel_max(delta, ref["delta"]) <= 1e-5
    s1, m1, max1 = t.read()
    prio = [float(abs(d)) + EPS for d in delta]
    assert max1 == max([max0] + prio)
    want = {int(sl): p for sl, p in zip(slots, prio)}
    boot_only = set(boot.tolist()) - set(want)
    if b == 5:
        assert boot_only                                                   # some walk ends on a row that was not sampled
    for slot in range(CAP):
        if slot in want:
            p = want[slot] ** alpha
            assert abs(s1[t.cap2 + slot] - p) <= 1e-12 * p and m1[t.cap2 + slot] == s1[t.cap2 + slot], slot
        else:
            assert s1[t.cap2 + slot] == s0[t.cap2 + slot] and m1[t.cap2 + slot] == m0[t.cap2 + slot], slot
    P.assert_trees_follow_from_their_leaves(s1, m1)


@pytest.mark.parametrize("dueling,double", [(False, False), (True, True)])
@pytest.mark.parametrize("kind,b", [("mlp", 5), ("mlp", 32), ("cnn", 5)])
def test_net_dqn_step_n_with_one_step_is_the_one_step_entries_bit_for_bit(L, kind, b, dueling, double):
    a_dim = 2 if kind == "mlp" else 4
    spec, ospec = _spec_pair(kind, a_dim, dueling)
    net, target, _, _ = _nets(spec, ospec, dueling)
    ring, _, _, _ = _filled_replay(kind, net, a_dim)
    rng = np.random.default_rng(b)
    slots = torch.from_numpy(rng.permutation(CAP)[:b].astype(np.int32)).cuda()
    rings = (ring.cur_state, ring.next_state)
    labels = (ring.action, ring.reward, ring.done)
    out = net.dqn_step(target, *rings, slots, *labels, GAMMA, dueling, double).clone()
    grads = net.grads.clone()
    net.grads.zero_()
    out_n = net.dqn_step(target, *rings, slots, *labels, GAMMA, dueling, double, ring.follow, 1).clone()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out_n), _bits(out)) and torch.equal(_bits(net.grads), _bits(grads))
    assert bool(grads.any()) and torch.equal(net.nstep_boot[:b], slots)
    # prioritised: two equal sets of trees
    u = torch.from_numpy(rng.random(b)).cuda()
    ta, tb = _primed_trees(CAP, 0.6, np.random.default_rng(1)), _primed_trees(CAP, 0.6, np.random.default_rng(1))
    assert torch.equal(ta.sum, tb.sum)
    out = net.dqn_step(target, *rings, None, *labels, GAMMA, dueling, double, per=_per_kw(ta, u)).clone()
    grads = net.grads.clone()
    net.grads.zero_()
    out_n = net.dqn_step(target, *rings, None, *labels, GAMMA, dueling, double, ring.follow, 1, per=_per_kw(tb, u)).clone()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out_n), _bits(out)) and torch.equal(_bits(net.grads), _bits(grads))
    assert torch.equal(_bits(tb.sum), _bits(ta.sum)) and torch.equal(_bits(tb.min), _bits(ta.min))
    assert torch.equal(_bits(tb.max_prio), _bits(ta.max_prio))
    assert not torch.equal(ta.sum, _primed_trees(CAP, 0.6, np.random.default_rng(1)).sum)            # the step wrote the trees


def test_net_dqn_step_n_refusals_change_no_buffer(L):
    from xingtian_amd import lib as LL
    spec, ospec = _spec_pair("mlp", 2, False)
    net, target, _, _ = _nets(spec, ospec, False, max_batch=8)
    ring, _, _, _ = _filled_replay("mlp", net, 2)
    slots = torch.tensor([3, 49, 7, 20], dtype=torch.int32, device="cuda")
    t = _primed_trees(CAP, 0.6, np.random.default_rng(0))
    u = torch.full((4,), 0.5, dtype=torch.float64, device="cuda")
    labels = (ring.action, ring.reward, ring.done)
    net.dqn_step(target, ring.cur_state, ring.next_state, None, *labels, GAMMA, False, False, ring.follow, 3,
                 per=_per_kw(t, u))                                         # allocates every scratch buffer; a good call
    torch.cuda.synchronize()
    _, row_bytes, cfg = net._dqn_cfg("test", ring.cur_state, ring.next_state, {"slots": slots}, *labels, GAMMA, False, False)
    _, per = net._per_cfg("test", u, t.sum, t.min, t.max_prio, 0.6, 0.4, EPS)
    scratch = [net.nstep_boot, net.nstep_action, net.nstep_reward, net.nstep_disc, net.nstep_done]
    watched = scratch + [net.grads, net.loss_out, net.per_slots, net.per_weights, t.sum, t.min, t.max_prio,
                         net._dqn_scratch[0], net._dqn_scratch[1], net._dqn_scratch[2], ring.follow]
    net.per_slots.fill_(-3)                                                # a refused call must not even sample
    before = [x.clone() for x in watched]

    def call(n=3, follow=ring.follow, null=None, with_per=False):
        ptrs = [None if null == i else x.data_ptr() for i, x in enumerate(scratch)]
        ns = LL.NstepCfg(n, None if follow is None else follow.data_ptr(), *ptrs)
        return net.lib.xt_net_dqn_step_n(net.handle, target.handle, ctypes.byref(cfg), ctypes.byref(ns),
                                         ctypes.byref(per) if with_per else None, LL.ptr(ring.cur_state),
                                         LL.ptr(ring.next_state), row_bytes, CAP, CAP, None if with_per else LL.ptr(slots), 4,
                                         *(LL.ptr(x) for x in labels), LL.ptr(net.loss_out), None, LL.stream_ptr())

    cases = [(dict(n=0), "outside [1, 256]"), (dict(n=257), "outside [1, 256]"), (dict(follow=None), "follow")]
    cases += [(dict(null=i), "null scratch") for i in range(5)]
    for with_per in (False, True):
        for kw, word in cases:
            assert call(with_per=with_per, **kw) != 0, kw
            msg = L.load().xt_last_error().decode()
            assert "xt_net_dqn_step_n" in msg and word in msg, (kw, msg)
    rc = net.lib.xt_net_dqn_step_n(net.handle, target.handle, ctypes.byref(cfg), None, None, LL.ptr(ring.cur_state),
                                   LL.ptr(ring.next_state), row_bytes, CAP, CAP, LL.ptr(slots), 4,
                                   *(LL.ptr(x) for x in labels), LL.ptr(net.loss_out), None, LL.stream_ptr())
    assert rc != 0 and "null nstep cfg" in L.load().xt_last_error().decode()
    net.set_dp(0, 2)                                                       # a data-parallel tail
    for with_per in (False, True):
        assert call(with_per=with_per) != 0
        assert "data parallelism" in L.load().xt_last_error().decode()
    with pytest.raises(RuntimeError) as info:
        net.dqn_step(target, ring.cur_state, ring.next_state, slots, *labels, GAMMA, False, False, ring.follow, 3)
    assert "data parallelism" in str(info.value) and "xt_net_dqn_step_n" in str(info.value)
    torch.cuda.synchronize()
    for x, was in zip(watched, before):
        assert torch.equal(_bits(x), _bits(was))


# ------------------------------------------------------------------------------------------------ alg_builder("DQN")
def _build(kind, a_dim, dueling, double, batch, **extra):
    from xingtian_amd.algorithm import alg_builder
    mc = {"dueling": dueling, "SEED": 3, "LR": 3e-4}
    if kind == "mlp":
        mc.update(HIDDEN_SIZE=32, NUM_LAYERS=1)
    info = {"actor": {"model_name": "DqnCnn" if kind == "cnn" else "DqnMlp", "type": "learner",
                      "state_dim": [84, 84, 4] if kind == "cnn" else [4], "action_dim": a_dim, "model_config": mc}}
    cfg = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1, "BUFFER_SIZE": CAP, "BATCH_SIZE": batch,
           "TARGET_UPDATE_FREQ": 3, "GAMMA": GAMMA, "double_dqn": double}
    cfg.update(extra)
    return alg_builder("DQN", info, cfg)


@pytest.mark.parametrize("kind,dueling,double,batch,prioritised", [("mlp", True, True, 32, False),
                                                                   ("cnn", False, False, 8, True)])
def test_dqn_algorithm_with_n_step_four_trains_against_the_oracle(L, kind, dueling, double, batch, prioritised):
    """The bars are those of test_dqn_algorithm_four_trains_target_cadence_restore_and_replica, used where it uses them:
    the single-step bars (loss 1e-4, every gradient tensor 1e-5) on the first train, where both sides hold the same
    weights, and after the fourth train every tensor's change within 3x the float32 oracle's own deviation from float64.
    The loss of every train is held to 1e-4 as well."""
    from xingtian_amd.algorithm.dqn.dqn import PrioritizedDeviceReplay, nstep_targets
    a_dim = 2 if kind == "mlp" else 4
    spec, ospec = _spec_pair(kind, a_dim, dueling)
    extra = dict(prioritized_replay=True) if prioritised else {}
    alg = _build(kind, a_dim, dueling, double, batch, n_step=3, **extra)
    assert alg.device_step and alg.n_step == 3 and alg.buff.n_step == 3
    assert (type(alg.buff) is PrioritizedDeviceReplay) == prioritised
    store = N.BruteStore(CAP)
    msgs = N.make_messages(CAP, 11, a_dim=a_dim, states=_state_fn(kind), reward_shift=2.0)
    for m in msgs:
        alg.prepare_data(m)
        store.add(m)
    buf = alg.buff
    row_bytes = buf.cur_state[0].numel() * buf.cur_state.element_size()
    assert buf.bytes == CAP * (2 * row_bytes + 17) + (2 * 2 * 64 * 8 if prioritised else 0)
    assert buf.follow.cpu().tolist() == store.follow()
    cur = {s: msgs[m]["cur_state"][t] for s, (m, t) in enumerate(store.slot)}
    nxt = {s: msgs[m]["next_state"][t] for s, (m, t) in enumerate(store.slot)}
    p_on, p_tg = H.seeded_params(ospec, 1, dueling), H.seeded_params(ospec, 2, dueling)
    alg.actor.set_weights(H.to_keras_names(spec, ospec, p_on))
    alg.target_actor.set_weights(H.to_keras_names(spec, ospec, p_tg))
    net = alg.actor.net
    net.lib = N.CountingLib(net.lib)
    clip = 10.0 if kind == "cnn" else None
    copy = lambda p: {k: v.copy() for k, v in p.items()}
    orc = H.DqnOracle(ospec, copy(p_on), copy(p_tg), dueling, double, GAMMA, 3e-4, clip, np.float64)
    orc32 = H.DqnOracle(ospec, copy(p_on), copy(p_tg), dueling, double, GAMMA, 3e-4, clip, np.float32)
    rng = np.random.default_rng(17)
    if prioritised:                                                        # the first train's draw on the fresh trees
        fresh = P.build_trees([1.0] * CAP + [0.0] * (64 - CAP))

        def draw(seed=[4]):
            seed[0] += 1
            random.seed(seed[0])
            return P.sample(*fresh, CAP, [random.random() for _ in range(batch)], 0.4)[1], seed[0]
        first, seed = _well_conditioned(kind, a_dim, draw)
        random.seed(seed)
    else:
        first, _ = _well_conditioned(kind, a_dim, lambda: (buf.slots_of(rng.permutation(CAP)[:batch]), None))
    target_init = alg.target_actor.net.params.clone()
    for t in range(1, 5):
        if prioritised:
            loss = alg.train()
            slots, w = net.per_slots[:batch].cpu().numpy(), net.per_weights[:batch].cpu().numpy()
        else:
            slots, w = np.asarray(first if t == 1 else buf.slots_of(rng.permutation(CAP)[:batch])), None
            loss = alg.train_on_slots(slots.tolist())
        if t == 1:
            assert slots.tolist() == list(first)
        boot, act_n, rew_n, disc_n, done_n = nstep_targets(slots, *N.host_rings(buf), GAMMA, 3, CAP)
        brute, _ = store.targets(slots.tolist(), 3)
        for got, want in zip((boot, act_n, rew_n, disc_n, done_n), brute):
            assert np.array_equal(got, want)
        batch_args = (np.stack([cur[s] for s in slots]), np.stack([nxt[j] for j in boot]), act_n, rew_n, done_n, w, disc_n)
        if t == 1:
            _assert_step(loss, net.grads_dict(), orc.step(*batch_args, apply=False), spec, ospec)
        ref = orc.step(*batch_args, apply=True)
        orc32.step(*batch_args, apply=True)
        print("dqn n-step train", t, "loss", loss, float(ref["loss"]))
        assert abs(loss - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"])), (t, loss, ref["loss"])
        if t % 3 == 0:
            orc.sync_target()
            orc32.sync_target()
        tp = alg.target_actor.net.params
        assert torch.equal(tp, target_init) if t < 3 else (torch.equal(tp, alg.actor.net.params) == (t == 3))
    assert alg.train_count == 4 and alg.actor.iterations == 4
    w4, report = alg.get_weights(), {}
    for h, o in H.name_map(spec, ospec).items():
        r = orc.net.params[o]
        d64 = r - np.asarray(p_on[o], np.float64)
        nrm = np.linalg.norm(d64) + 1e-30
        gpu = np.linalg.norm(w4[h].reshape(r.shape) - np.asarray(p_on[o], np.float64) - d64) / nrm
        f32 = np.linalg.norm(orc32.net.params[o].astype(np.float64) - np.asarray(p_on[o], np.float64) - d64) / nrm
        report[h] = (float(gpu), float(f32))
    print("dqn n-step four trains, per tensor (gpu, oracle32) deviation of the weight change:", report)
    for h, (gpu, f32) in report.items():
        assert gpu <= 3.0 * f32, (h, gpu, f32)
    calls = net.lib.calls
    assert calls["xt_net_dqn_step_n"] == 4 and calls["xt_net_dqn_step"] == 0 and calls["xt_net_dqn_step_per"] == 0


@pytest.mark.parametrize("prioritised", [False, True])
def test_dqn_without_n_step_never_calls_the_new_entry(L, prioritised):
    alg = _build("mlp", 2, False, False, 8, **(dict(prioritized_replay=True) if prioritised else {}))
    assert alg.n_step == 1
    for m in N.make_messages(CAP, 11, a_dim=2, states=_state_fn("mlp")):
        alg.prepare_data(m)
    assert alg.buff.follow is None
    net = alg.actor.net
    net.lib = N.CountingLib(net.lib)
    random.seed(1)
    for _ in range(2):
        alg.train()
    torch.cuda.synchronize()
    calls = net.lib.calls
    assert calls["xt_net_dqn_step_n"] == 0 and calls["xt_net_dqn_step_per" if prioritised else "xt_net_dqn_step"] == 2
    assert not hasattr(net, "nstep_boot")
