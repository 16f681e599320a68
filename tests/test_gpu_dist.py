"""GPU tests of the distributional (C51) DQN path: the head ``xt_dqn_loss_dist`` alone against the float64 restatement
(bars: four times the float32 NumPy restatement's own deviation, ``dist_helpers.head_bars``), heads wider than one
workgroup, ``xt_net_dqn_step_dist`` against the float64 checker (uniform, prioritised, n-step, both, double DQN) at the
project's standing bars (loss 1e-4, every gradient tensor 1e-5 by ``rel_max``), and ``alg_builder("DQN")`` with
``model_config.atoms``."""
import ctypes

import numpy as np
import pytest
import torch

import dist_helpers as D
import dqn_helpers as H
import nstep_helpers as N
import per_helpers as P

pytestmark = pytest.mark.gpu

GAMMA = D.GAMMA
EPS = 1e-6
CAP = 50
V_MIN, V_MAX = -10.0, 10.0


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
@pytest.mark.parametrize("shape", D.HEAD_SHAPES, ids=["B%d_A%d_N%d" % s for s in D.HEAD_SHAPES])
def test_dqn_loss_dist_against_float64(L, shape, double, weighted, with_disc, through_slots):
    b, a, n = shape
    c = D.head_case(shape, double, weighted, with_disc, through_slots)
    ref = D.head_ref(c)
    pl = c["planted"]
    gap = D.argmax_gap(ref, pl, c["v_max"] - c["v_min"])
    assert gap >= 1e-4, gap                                   # the condition under which a* is comparable at all
    rc, got = D.gpu_dqn_loss_dist(c)
    assert rc == 0
    measured, bars = D.head_bars()
    terms = got["out"][4:].reshape(b, 2)
    errs = {"m": H.rel_max(got["m"], ref["m"]), "loss_b": H.rel_max(terms[:, 0], ref["loss_b"]),
            "dlogits": H.rel_max(got["dlogits"], ref["dlogits"]), "qstar": H.rel_max(got["maxq"], ref["qstar"])}
    print("dist head", shape, (double, weighted, with_disc, through_slots), "errs", errs, "bars", bars)
    assert np.array_equal(got["astar"], ref["astar"])
    if "tie" in pl and a > 1:
        assert got["astar"][pl["tie"]] == 0                   # identical picking logits: the first index wins
    for k, e in errs.items():
        assert e <= bars[k], (k, e, bars[k])
    assert np.array_equal(terms[:, 1], got["maxq"])
    # every column outside the taken action's atoms, and dvalue: exactly 0 (written by the kernel over the NaN sentinels)
    taken = np.zeros((b, a, n), bool)
    taken[np.arange(b), ref["act"]] = True                    # (actions -1 and A are clamped into [0, A))
    dl = got["dlogits"].reshape(b, a, n)
    assert not np.isnan(dl).any() and (dl[~taken] == 0).all() and (got["dvalue"] == 0).all()
    if "done" in pl:
        assert ref["act"][pl["done"]] == 0                    # action -1 lands on action 0
    if "clamp_hi" in pl:
        assert ref["act"][pl["clamp_hi"]] == a - 1
        m_hi = got["m"][pl["clamp_hi"]]
        assert not m_hi[:-1].any() and abs(m_hi[-1] - 1.0) <= 1e-6               # all mass on the last atom
    if "clamp_lo" in pl:
        m_lo = got["m"][pl["clamp_lo"]]
        assert not m_lo[1:].any() and abs(m_lo[0] - 1.0) <= 1e-6
    if "integer" in pl and with_disc:                         # g = 1, R = 0, delta = 0.5: every b_j an integer, m is p bit for bit
        tl = c["t_logits"].reshape(b, a, n)[pl["integer"], got["astar"][pl["integer"]]].astype(np.float64)
        e = np.exp(tl - tl.max())
        p64 = e / e.sum()
        assert abs(float(got["m"][pl["integer"]].sum()) - 1.0) <= 1e-6
        assert np.abs(got["m"][pl["integer"]] - p64).max() <= 4 * 2.0 ** -24     # m is a float32 softmax there
    # the means: the kernel's own terms reduced in float64, to float32 rounding
    w = np.ones(b) if c["weights"] is None else c["weights"].astype(np.float32).astype(np.float64)
    t64 = terms.astype(np.float64)
    want = np.array([(w * t64[:, 0]).sum() / b, t64[:, 0].mean(), t64[:, 1].mean()])
    assert np.abs(got["out"][:3] - want).max() <= 2.0 ** -23 * max(1.0, np.abs(want).max())
    assert abs(got["out"][0] - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"]))


def test_dqn_loss_dist_integer_row_carries_the_target_softmax_bit_for_bit_and_m_is_optional(L):
    """g = 1, R = 0 on a support with delta = 0.5: every b_j is the integer j, so m_i = (float)((double)p_i * 1.0) = p_i.
    The kernel does not hand p out, so the bits are compared between two of its own projections of the same p: the
    identity, and the shift by exactly one atom (R = delta), where m_i = p_{i-1}, the last atom takes p_{N-2} + p_{N-1}
    (added in float64, rounded once) and the first atom takes nothing."""
    c = D.head_case((7, 2, 51), False, False, True, False)
    row = c["planted"]["integer"]
    rc, got = D.gpu_dqn_loss_dist(c)
    assert rc == 0
    c2 = dict(c, reward=c["reward"].copy())
    c2["reward"][row] = 0.5
    rc, got2 = D.gpu_dqn_loss_dist(c2)
    assert rc == 0
    m0, m1 = got["m"][row], got2["m"][row]
    assert np.array_equal(m1[1:-1], m0[:-2]) and m1[0] == 0.0
    assert m1[-1] == np.float32(np.float64(m0[-2]) + np.float64(m0[-1]))
    rc, got3 = D.gpu_dqn_loss_dist(c, want_m=False)
    assert rc == 0 and np.isnan(got3["m"]).all() and np.array_equal(got3["dlogits"], got["dlogits"])


# ------------------------------------------------------------------------------------------------ networks and replay
def _state_fn(kind):
    if kind == "cnn":
        return lambda tags, nxt: np.random.default_rng(int(tags[0]) * 2 + nxt).integers(
            0, 256, (len(tags), 84, 84, 4), dtype=np.uint8)
    return lambda tags, nxt: np.random.default_rng(int(tags[0]) * 2 + nxt).standard_normal((len(tags), 4)).astype(np.float32)


def _nets(spec, ospec, max_batch=33, mark=True):
    from xingtian_amd.model.hip_net import HipActorCritic
    p_on, p_tg = H.seeded_params(ospec, 1, False), H.seeded_params(ospec, 2, False)
    net, target = HipActorCritic(spec, max_batch=max_batch, seed=0), HipActorCritic(spec, max_batch=max_batch, seed=0)
    net.set_weights(H.to_keras_names(spec, ospec, p_on))
    target.set_weights(H.to_keras_names(spec, ospec, p_tg))
    if mark:
        net.set_dist(spec.atoms, V_MIN, V_MAX)
        target.set_dist(spec.atoms, V_MIN, V_MAX)
    return net, target, p_on, p_tg


def _filled_replay(kind, net, a_dim, n_step):
    from xingtian_amd.algorithm.dqn.dqn import DeviceReplay
    ring = DeviceReplay(CAP, net.device, net.to_device_obs, n_step=n_step)
    store, msgs = N.fill(ring, CAP, 11, a_dim=a_dim, states=_state_fn(kind))
    cur = {s: msgs[m]["cur_state"][t] for s, (m, t) in enumerate(store.slot)}
    nxt = {s: msgs[m]["next_state"][t] for s, (m, t) in enumerate(store.slot)}
    return ring, store, cur, nxt


MARGIN = 1e-6
_MARGINS = {}


def _kink_margins(kind, width, ospec, p_on):
    """slot -> the smallest |pre-activation| of any ReLU unit in the float64 forward of the online net on that slot's
    state row.  A unit closer to zero than float32's accumulation error may come out on the other side of the kink in any
    float32 implementation, which no kernel accuracy can mend (tests/test_gpu_nstep.py): the minibatches are drawn among
    the rows that keep MARGIN from it."""
    if (kind, width) not in _MARGINS:
        from oracle import nets
        msgs, store = N.make_messages(CAP, 11, a_dim=2, states=_state_fn(kind)), N.BruteStore(CAP)
        for m in msgs:
            store.add(m)
        net = nets.ActorCritic(ospec, p_on, np.float64)
        net.forward(np.stack([msgs[m]["cur_state"][t] for m, t in store.slot]))
        _MARGINS[(kind, width)] = np.min([np.abs(z.reshape(CAP, -1)).min(1) for _, _, z in net.cache[0]], axis=0)
    return _MARGINS[(kind, width)]


_GAPS = {}


def _argmax_gaps(kind, a, n, ospec, p_pick, which):
    """slot -> gap between the two best dist_q (float64, relative to v_max - v_min) of the picking net on that slot's
    next-state row: the argmax-stability condition, evaluated on the restatement alone for every row of the table.
    ``which`` names the parameter set (the seeds are fixed: "online" is seed 1, "target" seed 2) for the cache."""
    key = (kind, a, n, which)
    if key not in _GAPS:
        from oracle import nets
        msgs, store = N.make_messages(CAP, 11, a_dim=2, states=_state_fn(kind)), N.BruteStore(CAP)
        for m in msgs:
            store.add(m)
        lg, _ = nets.ActorCritic(ospec, p_pick, np.float64).forward(np.stack([msgs[m]["next_state"][t] for m, t in store.slot]))
        lg = lg.reshape(CAP, a, n)
        e = np.exp(lg - lg.max(-1, keepdims=True))
        q = np.sort((D.support(n, V_MIN, V_MAX)[0] * e).sum(-1) / e.sum(-1), axis=1)
        _GAPS[key] = (q[:, -1] - q[:, -2]) / (V_MAX - V_MIN) if a > 1 else np.full(CAP, np.inf)
    return _GAPS[key]


def _ok_slots(kind, a, n, ospec, p_on, p_pick, which, boot_of=lambda s: s):
    """-> the slots whose state row keeps MARGIN from the kink and whose bootstrap row keeps the two best dist_q of the
    picking net 2e-4 (v_max - v_min) apart (twice the condition the tests assert on their own reference).  With the
    near-uniform distributions of a freshly initialised network a fifth of the 84x84 rows miss the second condition, so
    the minibatches are drawn among these slots instead of being redrawn until they fit."""
    margins, gaps = _kink_margins(kind, a * n, ospec, p_on), _argmax_gaps(kind, a, n, ospec, p_pick, which)
    every = np.arange(CAP)
    return np.flatnonzero((margins >= MARGIN) & (gaps[np.asarray(boot_of(every))] >= 2e-4)).astype(np.int32)


# ------------------------------------------------------------------------------------------------ wide heads
WIDE = [(2, 2), (2, 51), (5, 51), (2, 128), (2, 129), (6, 51)]          # widths 4, 102, 255, 256, 258, 306


@pytest.mark.parametrize("wide", [True, False], ids=["wide", "generic"])
@pytest.mark.parametrize("b", [1, 7, 33])
@pytest.mark.parametrize("a,n", WIDE, ids=["W%d" % (a * n) for a, n in WIDE])
def test_wide_heads_forward_and_every_gradient_tensor_against_float64(L, a, n, b, wide):
    """On the head kernels of a marked net (``wide``) and on those every other net runs (``set_dist_wide(False)``).  Widths 256 and above are the ones the one-thread-per-bias write of the head weight gradient left unwritten.  257 is
    a prime, so no distributional net (atoms >= 2) has it: 258 stands in for it through the step, and 257 itself is
    covered on the head entries below."""
    spec, ospec = D.spec_pair("mlp", a, n)
    assert spec.action_dim == a * n
    net, target, p_on, p_tg = _nets(spec, ospec)
    net.set_dist_wide(wide)
    target.set_dist_wide(wide)
    ring, store, cur, nxt = _filled_replay("mlp", net, a, 1)
    rng = np.random.default_rng(a * n + b)
    slots = rng.permutation(_ok_slots("mlp", a, n, ospec, p_on, p_on, "online"))[:b]
    assert len(slots) == b
    orc = D.DistOracle(ospec, p_on, p_tg, a, n, V_MIN, V_MAX, True, 3e-4)
    act, rew, done = (x.cpu().numpy()[slots] for x in (ring.action, ring.reward, ring.done))
    states, nstates = np.stack([cur[s] for s in slots]), np.stack([nxt[s] for s in slots])
    ref = orc.step(states, nstates, act, rew, np.full(b, GAMMA), done)
    logits = net.forward(states)[0].cpu().numpy()
    # 32 float32 products per logit: the error is at most 32 * 2^-24 = 2e-6 of sum |f w|, itself a few times the largest logit
    assert logits.shape == (b, a * n) and H.rel_max(logits, ref["logits"]) <= 1e-5
    net.grads.fill_(float("nan"))
    out = net.dqn_step(target, ring.cur_state, ring.next_state, torch.from_numpy(slots).cuda(), ring.action,
                       ring.reward, ring.done, GAMMA, False, True, dist=True)
    torch.cuda.synchronize()
    grads = net.grads_dict()
    for k, g in grads.items():
        assert np.isfinite(g).all(), k                        # (an unwritten bias gradient keeps its NaN)
    D.assert_step(float(out.cpu().numpy()[0]), grads, ref, spec, ospec, "wide %d B %d" % (a * n, b))


@pytest.mark.parametrize("b", [1, 7, 33])
def test_width_257_forward_and_head_weight_gradient_slabs_against_float64(L, b):
    from xingtian_amd.model import netspec
    width, F = 257, 32
    spec, ospec = netspec.dqn_mlp((4,), width, F, 1), H.oracle_spec("mlp", (4,), width, F, 1)
    net, _, p_on, _ = _nets(spec, ospec, mark=False)
    from oracle import nets
    rng = np.random.default_rng(b)
    x = rng.standard_normal((b, 4)).astype(np.float32)
    want, _ = nets.ActorCritic(ospec, p_on, np.float64).forward(x)
    assert H.rel_max(net.forward(x)[0].cpu().numpy(), want) <= 1e-5
    feat = rng.standard_normal((b, F)).astype(np.float32)
    dl, dv = rng.standard_normal((b, width)).astype(np.float32), rng.standard_normal(b).astype(np.float32)
    chunks = (b + 7) // 8
    st_pi, st_v = F * width + width + 3, F + 1 + 3
    up = lambda v: torch.from_numpy(v).cuda()
    slab_pi = torch.full((chunks * st_pi,), float("nan"), device="cuda")
    slab_v = torch.full((chunks * st_v,), float("nan"), device="cuda")
    d_f, d_dl, d_dv, nchunk = up(feat), up(dl), up(dv), ctypes.c_int32(-1)
    L.check(L.load().xt_heads_wgrad_partial_ex(L.ptr(d_f), L.ptr(d_f), b, F, width, L.ptr(d_dl), L.ptr(d_dv), L.ptr(slab_pi),
                                               st_pi, L.ptr(slab_v), st_v, ctypes.byref(nchunk), None), "wgrad 257")
    torch.cuda.synchronize()
    assert nchunk.value == chunks
    spi, sv = slab_pi.cpu().numpy().reshape(chunks, st_pi), slab_v.cpu().numpy().reshape(chunks, st_v)
    assert np.isnan(spi[:, F * width + width:]).all() and np.isnan(sv[:, F + 1:]).all()
    assert np.isfinite(spi[:, :F * width + width]).all() and np.isfinite(sv[:, :F + 1]).all()       # every bias sum written
    s_pi, s_v = spi[:, :F * width + width].astype(np.float64).sum(0), sv[:, :F + 1].astype(np.float64).sum(0)
    f64, dl64, dv64 = feat.astype(np.float64), dl.astype(np.float64), dv.astype(np.float64)
    assert H.rel_max(s_pi[:F * width].reshape(F, width), f64.T @ dl64) <= 1e-5
    assert H.rel_max(s_pi[F * width:], dl64.sum(0)) <= 1e-5
    assert H.rel_max(s_v[:F], f64.T @ dv64) <= 1e-5 and H.rel_max(s_v[F:], dv64.sum(keepdims=True)) <= 1e-5


# ------------------------------------------------------------------------------------------------ the whole step
def _primed_trees(size, alpha, rng, ok):
    """trees whose leaves of the slots in ``ok`` hold priorities in [0.01, 3] and the others eps: a draw of 32 then stays
    among ``ok`` with probability 0.999"""
    t = P.GpuTrees(CAP, alpha)
    assert t.add(0, size) == 0
    delta = np.zeros(size, np.float32)
    delta[ok] = rng.uniform(0.01, 3.0, len(ok))
    assert t.update(list(range(size)), delta, EPS) == 0
    return t


STEP_VARIANTS = {"uniform": (False, 1, False), "per": (True, 1, False), "nstep": (False, 3, False),
                 "per_nstep": (True, 3, False), "double": (False, 1, True)}


@pytest.mark.parametrize("wide", [True, False], ids=["wide", "generic"])
@pytest.mark.parametrize("variant", list(STEP_VARIANTS))
@pytest.mark.parametrize("kind", ["mlp", "cnn"])
def test_net_dqn_step_dist_against_float64(L, kind, variant, wide):
    from xingtian_amd.algorithm.dqn.dqn import nstep_targets
    prioritised, n_step, double = STEP_VARIANTS[variant]
    b, atoms, alpha, beta = 32, 51, 0.6, 0.4
    a_dim = 2 if kind == "mlp" else 4
    spec, ospec = D.spec_pair(kind, a_dim, atoms)
    net, target, p_on, p_tg = _nets(spec, ospec, 32)
    net.set_dist_wide(wide)
    target.set_dist_wide(wide)
    target_before = target.params.clone()
    ring, store, cur, nxt = _filled_replay(kind, net, a_dim, n_step)
    rng = np.random.default_rng(len(variant) + 7 * (kind == "cnn"))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    if n_step > 1:
        labels = lambda s: nstep_targets(s, *N.host_rings(ring), GAMMA, n_step, CAP)
    else:
        h = lambda x: x.cpu().numpy()
        labels = lambda s: (np.asarray(s, np.int32), h(ring.action)[s], h(ring.reward)[s], np.full(len(s), GAMMA),
                            h(ring.done)[s])
    boot_of = lambda s: labels(s)[0]
    p_pick = p_on if double else p_tg
    kw = dict(follow=ring.follow, n=n_step, dist=True) if n_step > 1 else dict(dist=True)
    args = (ring.action, ring.reward, ring.done, GAMMA, False, double)
    ok = _ok_slots(kind, a_dim, atoms, ospec, p_on, p_pick, "online" if double else "target", boot_of)
    assert len(ok) >= b
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
    orc = D.DistOracle(ospec, p_on, p_tg, a_dim, atoms, V_MIN, V_MAX, double, 3e-4)
    ref = orc.step(np.stack([cur[s] for s in slots]), np.stack([nxt[j] for j in boot]), act, rew, disc, done, w)
    gap = D.argmax_gap(ref, {}, V_MAX - V_MIN)
    assert gap >= 1e-4, gap
    got = out.cpu().numpy()
    D.assert_step(float(got[0]), net.grads_dict(), ref, spec, ospec, "%s %s" % (kind, variant))
    assert abs(got[1] - ref["mean_loss"]) <= 1e-4 * max(1.0, ref["mean_loss"]) and abs(got[2] - ref["mean_q"]) <= 1e-4 * 10.0
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


def test_net_dqn_step_dist_refusals_and_the_scalar_entries_on_a_marked_net(L):
    spec, ospec = D.spec_pair("mlp", 2, 51)
    net, target, _, _ = _nets(spec, ospec, 8)
    ring, _, _, _ = _filled_replay("mlp", net, 2, 1)
    slots = torch.arange(4, dtype=torch.int32, device="cuda")
    args = (ring.cur_state, ring.next_state, slots, ring.action, ring.reward, ring.done, GAMMA)
    net.grads.zero_()
    with pytest.raises(RuntimeError, match="marked distributional"):
        net.dqn_step(target, *args, False, False)
    target.set_dist(51, V_MIN, 20.0)
    with pytest.raises(RuntimeError, match="same atoms and bounds"):
        net.dqn_step(target, *args, False, False, dist=True)
    target.set_dist(1, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="same atoms and bounds"):
        net.dqn_step(target, *args, False, False, dist=True)
    with pytest.raises(RuntimeError, match="no multiple of atoms"):
        target.set_dist(50, V_MIN, V_MAX)
    with pytest.raises(RuntimeError, match="finite v_min < v_max"):
        target.set_dist(51, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="not marked distributional"):
        target.set_dist_wide(True)
    torch.cuda.synchronize()
    assert not bool(net.grads.any())                          # nothing was launched
    target.set_dist(51, V_MIN, V_MAX)
    net.dqn_step(target, *args, False, False, dist=True)
    torch.cuda.synchronize()
    assert bool(net.grads.any())


# ------------------------------------------------------------------------------------------------ through the plugin pair
def test_dqn_algorithm_with_atoms_three_trains_against_the_oracle(L):
    from xingtian_amd.algorithm import alg_builder
    a_dim, atoms, batch = 2, 51, 32
    mc = {"atoms": atoms, "SEED": 3, "LR": 3e-4, "HIDDEN_SIZE": 32, "NUM_LAYERS": 1}
    info = {"actor": {"model_name": "DqnMlp", "type": "learner", "state_dim": [4], "action_dim": a_dim, "model_config": mc}}
    cfg = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1, "BUFFER_SIZE": CAP, "BATCH_SIZE": batch,
           "TARGET_UPDATE_FREQ": 2, "GAMMA": GAMMA, "double_dqn": False}
    alg = alg_builder("DQN", info, cfg)
    assert alg.device_step and alg.atoms == atoms and alg.actor.net.dist == (atoms, V_MIN, V_MAX)
    spec, ospec = D.spec_pair("mlp", a_dim, atoms)
    assert list(alg.actor.net.spec.names.items()) == list(spec.names.items())
    store = N.BruteStore(CAP)
    msgs = N.make_messages(CAP, 11, a_dim=a_dim, states=_state_fn("mlp"))
    for m in msgs:
        alg.prepare_data(m)
        store.add(m)
    cur = {s: msgs[m]["cur_state"][t] for s, (m, t) in enumerate(store.slot)}
    nxt = {s: msgs[m]["next_state"][t] for s, (m, t) in enumerate(store.slot)}
    p_on, p_tg = H.seeded_params(ospec, 1, False), H.seeded_params(ospec, 2, False)
    alg.actor.set_weights(H.to_keras_names(spec, ospec, p_on))
    alg.target_actor.set_weights(H.to_keras_names(spec, ospec, p_tg))
    net, buf = alg.actor.net, alg.buff
    net.lib = N.CountingLib(net.lib)
    copy = lambda p: {k: v.copy() for k, v in p.items()}
    orc = D.DistOracle(ospec, copy(p_on), copy(p_tg), a_dim, atoms, V_MIN, V_MAX, False, 3e-4)
    rng = np.random.default_rng(17)
    first = rng.permutation(_ok_slots("mlp", a_dim, atoms, ospec, p_on, p_tg, "target"))[:batch].tolist()
    target_init = alg.target_actor.net.params.clone()
    h = lambda x: x.cpu().numpy()
    for t in range(1, 4):
        slots = np.asarray(first if t == 1 else buf.slots_of(rng.permutation(CAP)[:batch]))
        loss = alg.train_on_slots(slots.tolist())
        batch_args = (np.stack([cur[s] for s in slots]), np.stack([nxt[s] for s in slots]), h(buf.action)[slots],
                      h(buf.reward)[slots], np.full(batch, GAMMA), h(buf.done)[slots])
        if t == 1:
            D.assert_step(loss, net.grads_dict(), orc.step(*batch_args), spec, ospec, "plugin train 1")
        ref = orc.step(*batch_args, apply=True)
        print("dist train", t, "loss", loss, float(ref["loss"]))
        assert abs(loss - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"])), (t, loss, ref["loss"])
        if t % 2 == 0:
            orc.sync_target()
        tp = alg.target_actor.net.params
        assert torch.equal(tp, target_init) if t < 2 else (torch.equal(tp, alg.actor.net.params) == (t == 2))
    assert alg.train_count == 3 and alg.actor.iterations == 3
    calls = net.lib.calls
    assert calls["xt_net_dqn_step_dist"] == 3 and calls["xt_net_dqn_step"] == 0 and calls["xt_net_dqn_step_n"] == 0
    x = np.stack([cur[s] for s in range(9)])
    q = alg.actor.predict(x)
    assert q.shape == (9, a_dim) and q.dtype == np.float32
    lg, _ = orc.net.forward(x)
    e = np.exp(lg.reshape(9, a_dim, atoms) - lg.reshape(9, a_dim, atoms).max(-1, keepdims=True))
    want = (D.support(atoms, V_MIN, V_MAX)[0] * e).sum(-1) / e.sum(-1)
    assert np.abs(q - want).max() <= 1e-4 * (V_MAX - V_MIN)
