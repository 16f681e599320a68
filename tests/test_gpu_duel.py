"""GPU tests of the dueling distributional heads (``dist_dueling``): the head entries ``xt_dqn_loss_dist_duel`` /
``xt_dqn_loss_quant_duel`` alone against the float64 restatement (bars: four times the float32 NumPy restatement's own
deviation, ``duel_helpers.head_bars``), exact checks on the kernels' own outputs, the feature-gradient kernel alone, and
``xt_net_dqn_step_dist`` / ``_quant`` on nets marked by ``xt_net_set_duel`` against the float64 checker (folded widths round
the 256-column block edge on both feature-gradient kernels; uniform, prioritised, n-step, both, double DQN; noisy layers)
at the project's standing bars (loss 1e-4, every gradient tensor 1e-5 by ``rel_max``), the refusals, and
``alg_builder("DQN")`` with ``model_config.dist_dueling``."""
import re

import numpy as np
import pytest
import torch

import dqn_helpers as H
import duel_helpers as U
import nstep_helpers as N
import per_helpers as P

pytestmark = pytest.mark.gpu

GAMMA = U.GAMMA
EPS = 1e-6
CAP = U.CAP


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
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the heads alone
@pytest.mark.parametrize("through_slots", [False, True])
@pytest.mark.parametrize("with_disc", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("shape", U.HEAD_SHAPES, ids=["B%d_A%d_N%d" % s for s in U.HEAD_SHAPES])
@pytest.mark.parametrize("head", U.HEADS)
def test_duel_head_against_float64(L, head, shape, double, weighted, with_disc, through_slots):
    b, a, n = shape
    c = U.head_case(head, shape, double, weighted, with_disc, through_slots)
    ref = U.head_ref(c)
    pl = c["planted"]
    gap = U.argmax_gap(c, ref)
    assert gap >= U.min_gap(head), gap                        # the condition under which a* is comparable at all
    rc, got = U.gpu_head(c)
    assert rc == 0
    U.assert_pads_untouched(got, b)
    measured, bars = U.head_bars(head)
    terms = got["out"][4:4 + 2 * b].reshape(b, 2)
    got_q = dict(loss_b=terms[:, 0], dcols=got["dlogits"][:b], qstar=got["maxq"][:b], out=got["out"][:3], m=got["m"][:b])
    errs = {k: H.rel_max(got_q[k], U.quantity(ref, k)) for k in U.HEAD_QUANTITIES[head]}
    print("duel", head, "head", shape, (double, weighted, with_disc, through_slots), "errs", errs, "bars", bars)
    assert np.array_equal(got["astar"][:b], ref["astar"])
    for name in ("tie", "equal_adv"):
        if name in pl and a > 1:
            assert got["astar"][pl[name]] == 0                # identical combined picking rows: the first index wins
    for k, e in errs.items():
        assert e <= bars[k], (k, e, bars[k])
    assert np.array_equal(terms[:, 1], got["maxq"][:b])
    # the gradient row's structure, on the kernel's own bits: the value group is d_i, every untaken group is
    # d_i * (0 - inv_A), the taken one d_i * (1 - inv_A); the whole row is written; dvalue is exactly 0
    dl = got["dlogits"][:b].reshape(b, a + 1, n)
    assert not np.isnan(dl).any() and (got["dvalue"][:b] == 0).all()
    d = dl[:, a]
    inv_a = np.float32(1.0) / np.float32(a)
    for k in range(a):
        hot = (ref["act"] == k).astype(np.float32)[:, None]     # (actions -1 and A are clamped into [0, A))
        assert np.array_equal(_bits(dl[:, k]), _bits(d * (hot - inv_a))), k
    if "done" in pl:
        assert ref["act"][pl["done"]] == 0                    # action -1 lands on action 0
    for name in ("clamp_hi", "clamp"):
        if name in pl:
            assert ref["act"][pl[name]] == a - 1              # action A lands on action A - 1
    if head == "c51":
        if "clamp_hi" in pl:
            m_hi = got["m"][pl["clamp_hi"]]
            assert not m_hi[:-1].any() and abs(m_hi[-1] - 1.0) <= 1e-6
        if "clamp_lo" in pl:
            m_lo = got["m"][pl["clamp_lo"]]
            assert not m_lo[1:].any() and abs(m_lo[0] - 1.0) <= 1e-6
    # the means: the kernel's own terms reduced in float64, to float32 rounding
    w = np.ones(b) if c["weights"] is None else c["weights"].astype(np.float32).astype(np.float64)
    t64 = terms.astype(np.float64)
    want = np.array([(w * t64[:, 0]).sum() / b, t64[:, 0].mean(), t64[:, 1].mean()])
    assert np.abs(got["out"][:3] - want).max() <= 2.0 ** -23 * max(1.0, np.abs(want).max())
    assert abs(got["out"][0] - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"]))


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("n", [2, 51, 65, 256])
@pytest.mark.parametrize("head", U.HEADS)
def test_one_action_is_the_plain_head_on_the_value_columns_bit_for_bit(L, head, n, double):
    """A = 1: mean_i = adv[0, i], so adv - mean is exactly 0 and l[0, :] = v: loss_b, qstar (and m) and the value group's
    gradient are those of the entry without _duel on the dense value columns, and the advantage group's gradient is 0."""
    b = 9
    c = U.head_case(head, (b, 1, n), double, True, True, True, seed=3)
    rc, got = U.gpu_head(c)
    assert rc == 0
    dense = dict(c, a=1)
    for k in ("logits", "t_logits", "o_logits"):
        dense[k] = None if c[k] is None else np.ascontiguousarray(c[k][:, n:])
    rc, plain = U.gpu_head(dense, entry="xt_dqn_loss_dist" if head == "c51" else "xt_dqn_loss_quant")
    assert rc == 0
    dl = got["dlogits"][:b].reshape(b, 2, n)
    assert np.array_equal(_bits(dl[:, 1]), _bits(plain["dlogits"][:b])) and plain["dlogits"][:b].any()
    assert (dl[:, 0] == 0).all()
    assert np.array_equal(_bits(got["out"][:4 + 2 * b][[0, 1, 2]]), _bits(plain["out"][[0, 1, 2]]))
    assert np.array_equal(_bits(got["out"][4:4 + 2 * b]), _bits(plain["out"][4:4 + 2 * b]))
    assert np.array_equal(_bits(got["maxq"][:b]), _bits(plain["maxq"][:b])) and (got["astar"][:b] == 0).all()
    if head == "c51":
        assert np.array_equal(_bits(got["m"][:b]), _bits(plain["m"][:b]))
    U.assert_pads_untouched(got, b)


@pytest.mark.parametrize("head", U.HEADS)
def test_duel_head_entries_refuse_by_name_and_write_nothing(L, head):
    c = U.head_case(head, (7, 2, 51), False, False, False, False)
    who = "xt_dqn_loss_dist_duel" if head == "c51" else "xt_dqn_loss_quant_duel"
    for kw, text in ((dict(a=64), "1 <= A <= 63"), (dict(a=0), "1 <= A <= 63"), (dict(b=0), "bad sizes"),
                     (dict(n=1), "outside \\[2, 256\\]"), (dict(n=257), "outside \\[2, 256\\]")):
        rc, got = U.gpu_head(c, **kw)
        err = L.load().xt_last_error().decode()
        assert rc != 0 and who in err and re.search(text, err), (kw, err)
        assert np.isnan(got["dlogits"]).all() and np.isnan(got["out"]).all()


# ------------------------------------------------------------------------------------------------ the feature gradient
DFEAT = [(1, 4, 1, 2), (7, 32, 2, 51), (33, 6, 6, 51), (5, 9, 18, 64), (5, 256, 3, 65), (3, 5, 2, 256), (66, 13, 4, 51)]


@pytest.mark.parametrize("through_slots", [False, True])
@pytest.mark.parametrize("b,f,a,n", DFEAT, ids=["B%d_F%d_A%d_N%d" % s for s in DFEAT])
def test_heads_dfeat_duel_against_float64(L, b, f, a, n, through_slots):
    """F below, at and off the four-feature tile; one, two and four columns per lane and a ragged last stride; more samples
    than one wave's share; a gradient row as the heads leave it (the structure the kernel relies on); ReLU features with
    zeros among them.  32..256 float32 products per sum: 1e-5 of the largest entry, the step's own bar."""
    rng = np.random.default_rng(b * f + a + n)
    w = a + 1
    feat = np.maximum(rng.standard_normal((b, f)), 0.0).astype(np.float32)
    wq = rng.standard_normal((f, w * n)).astype(np.float32)
    act = rng.integers(0, a, b).astype(np.int32)
    act[0] = -1 if b > 1 else act[0]
    act[-1] = a                                             # (clamped into [0, A), as the heads clamp)
    d = rng.standard_normal((b, n)).astype(np.float32)
    clamped = np.clip(act, 0, a - 1)
    dl = np.zeros((b, a, n), np.float32)
    dl[np.arange(b), clamped] = d
    dcols = U.combine_grad(dl.reshape(b, -1), clamped, a, n, np.float32)
    slots = rng.permutation(b + 5)[:b].astype(np.int32) if through_slots else None
    ring = act
    if through_slots:
        ring = np.full(b + 5, -7, np.int32)
        ring[slots] = act
    up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()
    d_feat, d_wq, d_dl, d_slots, d_act = up(feat), up(wq), up(dcols), up(slots), up(ring)
    out = torch.full((b + 2, f), float("nan"), dtype=torch.float32, device="cuda")
    rc = L.load().xt_heads_dfeat_duel(L.ptr(d_feat), b, f, a, n, L.ptr(d_wq), L.ptr(d_dl), L.ptr(d_slots), L.ptr(d_act), 1,
                                      L.ptr(out), L.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    got = out.cpu().numpy()
    assert np.isnan(got[b:]).all() and not np.isnan(got[:b]).any()
    want = (dcols.astype(np.float64) @ wq.astype(np.float64).T) * (feat > 0)
    assert H.rel_max(got[:b], want) <= 1e-5
    assert (got[:b][feat == 0] == 0).all()
    for kw in (dict(a=0), dict(a=64), dict(n=257), dict(b=0)):
        args = dict(b=b, f=f, a=a, n=n)
        args.update(kw)
        assert L.load().xt_heads_dfeat_duel(L.ptr(d_feat), args["b"], args["f"], args["a"], args["n"], L.ptr(d_wq), L.ptr(d_dl),
                                            L.ptr(d_slots), L.ptr(d_act), 1, L.ptr(out), L.stream_ptr()) != 0
        assert "xt_heads_dfeat_duel" in L.load().xt_last_error().decode()


# ------------------------------------------------------------------------------------------------ networks and replay
def _mark(net, head, n, duel=True):
    if head == "c51":
        net.set_dist(n, U.V_MIN, U.V_MAX)
    else:
        net.set_quant(n, U.KAPPA)
    if duel:
        net.set_duel(True)


def _nets(head, spec, ospec, max_batch=33, mark=True):
    from xingtian_amd.model.hip_net import HipActorCritic
    p_on, p_tg = H.seeded_params(ospec, 1, False), H.seeded_params(ospec, 2, False)
    net, target = HipActorCritic(spec, max_batch=max_batch, seed=0), HipActorCritic(spec, max_batch=max_batch, seed=0)
    net.set_weights(H.to_keras_names(spec, ospec, p_on))
    target.set_weights(H.to_keras_names(spec, ospec, p_tg))
    if mark:
        for x in (net, target):
            _mark(x, head, max(spec.atoms, spec.quantiles))
    return net, target, p_on, p_tg


def _filled_replay(kind, net, a_dim, n_step):
    from xingtian_amd.algorithm.dqn.dqn import DeviceReplay
    ring = DeviceReplay(CAP, net.device, net.to_device_obs, n_step=n_step)
    N.fill(ring, CAP, U.RING_SEED, a_dim=a_dim, states=U.state_fn(kind))
    return ring


def _kw(head, **more):
    return dict(dist=head == "c51", quant=head == "qr", **more)


# ------------------------------------------------------------------------------------------------ folded widths
WIDE = [(1, 2), (2, 51), (4, 51), (3, 64), (2, 86), (5, 51)]           # folded widths 4, 153, 255, 256, 258, 306


@pytest.mark.parametrize("wide", [True, False], ids=["duel_kernel", "generic"])
@pytest.mark.parametrize("b", [1, 7, 33])
@pytest.mark.parametrize("a,n", WIDE, ids=["W%d" % ((a + 1) * n) for a, n in WIDE])
@pytest.mark.parametrize("head", U.HEADS)
def test_folded_heads_forward_and_every_gradient_tensor_against_float64(L, head, a, n, b, wide):
    """On the kernels of a marked net (the wide forward, ``heads_dfeat_duel_kernel``) and, with ``set_dist_wide(False)``, on
    the generic forward and ``heads_dfeat_kernel``, which are right on a dense row as they stand: a same-run cross-check."""
    spec, ospec = U.spec_pair(head, "mlp", a, n)
    assert spec.action_dim == (a + 1) * n and spec.n_actions == a
    net, target, p_on, p_tg = _nets(head, spec, ospec)
    net.set_dist_wide(wide)
    target.set_dist_wide(wide)
    ring = _filled_replay("mlp", net, a, 1)
    _, _, cur, nxt = U.ring_rows("mlp", a)
    rng = np.random.default_rng((a + 1) * n + b)
    ok = U.ok_slots(head, "mlp", a, n, ospec, p_on, p_on, "online")
    orc = U.DuelOracle(head, ospec, p_on, p_tg, a, n, True, 3e-4)
    # A gradient tensor is compared relative to its own largest entry, and the head's bias gradient is the sum of the
    # gradient rows over the minibatch: where the rows cancel (two atoms, seven samples: down to 2 % of their size) the
    # comparison would measure the float32 forward against a near-zero tensor.  The minibatch is drawn, on the float64
    # oracle alone, among those whose column sums keep a fifth of the columns' absolute sums.
    for _ in range(50):
        slots = rng.permutation(ok)[:b]
        assert len(slots) == b
        act, rew, done = (x.cpu().numpy()[slots] for x in (ring.action, ring.reward, ring.done))
        ref = orc.step(cur[slots], nxt[slots], act, rew, np.full(b, GAMMA), done)
        if np.abs(ref["dcols"].sum(0)).max() >= 0.2 * np.abs(ref["dcols"]).sum(0).max():
            break
    else:
        raise AssertionError("no minibatch whose gradient rows do not cancel")
    logits = net.forward(cur[slots])[0].cpu().numpy()
    assert logits.shape == (b, (a + 1) * n) and H.rel_max(logits, ref["logits"]) <= 1e-5
    net.grads.fill_(float("nan"))
    out = net.dqn_step(target, ring.cur_state, ring.next_state, torch.from_numpy(slots).cuda(), ring.action, ring.reward,
                       ring.done, GAMMA, False, True, **_kw(head))
    torch.cuda.synchronize()
    grads = net.grads_dict()
    for k, g in grads.items():
        assert np.isfinite(g).all(), k
    U.assert_step(float(out.cpu().numpy()[0]), grads, ref, spec, ospec, "%s W%d B%d %s" % (head, (a + 1) * n, b, wide))


# ------------------------------------------------------------------------------------------------ the whole step
def _primed_trees(size, alpha, rng, ok):
    t = P.GpuTrees(CAP, alpha)
    assert t.add(0, size) == 0
    delta = np.zeros(size, np.float32)
    delta[ok] = rng.uniform(0.01, 3.0, len(ok))
    assert t.update(list(range(size)), delta, EPS) == 0
    return t


STEP_VARIANTS = {"uniform": (False, 1, False), "per": (True, 1, False), "nstep": (False, 3, False),
                 "per_nstep": (True, 3, False), "double": (False, 1, True)}


@pytest.mark.parametrize("variant", list(STEP_VARIANTS))
@pytest.mark.parametrize("kind", ["mlp", "cnn"])
@pytest.mark.parametrize("head", U.HEADS)
def test_net_dqn_step_duel_against_float64(L, head, kind, variant):
    prioritised, n_step, double = STEP_VARIANTS[variant]
    b, n, alpha, beta = 32, 51, 0.6, 0.4
    a_dim = 2 if kind == "mlp" else 4
    spec, ospec = U.spec_pair(head, kind, a_dim, n)
    net, target, p_on, p_tg = _nets(head, spec, ospec, 32)
    target_before = target.params.clone()
    ring = _filled_replay(kind, net, a_dim, n_step)
    _, _, cur, nxt = U.ring_rows(kind, a_dim)
    labels = U.host_labels(kind, a_dim, n_step)
    rng = np.random.default_rng(len(variant) + 7 * (kind == "cnn") + 3 * (head == "qr"))
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    kw = _kw(head, follow=ring.follow, n=n_step) if n_step > 1 else _kw(head)
    args = (ring.action, ring.reward, ring.done, GAMMA, False, double)
    ok = U.ok_slots(head, kind, a_dim, n, ospec, p_on, p_on if double else p_tg, "online" if double else "target", n_step)
    assert len(ok) >= b
    calls = net.lib = N.CountingLib(net.lib)
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
    assert calls.calls["xt_net_dqn_step_dist" if head == "c51" else "xt_net_dqn_step_quant"] == 1
    boot, act, rew, disc, done = labels(slots)
    if n_step > 1:
        assert (boot != slots).any() and len(set(disc.tolist())) > 1
    ref = U.DuelOracle(head, ospec, p_on, p_tg, a_dim, n, double, 3e-4).step(cur[slots], nxt[boot], act, rew, disc, done, w)
    assert U.ref_gap(head, ref) >= U.min_gap(head)
    got = out.cpu().numpy()
    U.assert_step(float(got[0]), net.grads_dict(), ref, spec, ospec, "%s %s %s" % (head, kind, variant))
    assert abs(got[1] - ref["mean_loss"]) <= 1e-4 * max(1.0, ref["mean_loss"])
    assert abs(got[2] - ref["mean_q"]) <= 1e-4 * max(10.0, abs(ref["mean_q"]))
    assert torch.equal(target.params, target_before) and not bool(target.grads.any())     # the target net is forward only
    if not prioritised:
        return
    # the leaves of the start slots take (loss_b + eps) ** alpha, formed on the host from the kernel's own terms
    loss_b = terms.cpu().numpy()[0::2]
    assert H.rel_max(loss_b, ref["loss_b"]) <= 1e-4 and (loss_b >= 0).all()
    s1, m1, max1 = t.read()
    prio = [float(abs(x)) + EPS for x in loss_b]
    assert max1 == max([max0] + prio)
    want = {int(sl): p for sl, p in zip(slots, prio)}         # (the last occurrence of a slot wins)
    for slot in range(CAP):
        if slot in want:
            p = want[slot] ** alpha
            assert abs(s1[t.cap2 + slot] - p) <= 1e-12 * p and m1[t.cap2 + slot] == s1[t.cap2 + slot], slot
        else:
            assert s1[t.cap2 + slot] == s0[t.cap2 + slot] and m1[t.cap2 + slot] == m0[t.cap2 + slot], slot
    P.assert_trees_follow_from_their_leaves(s1, m1)


@pytest.mark.parametrize("head", U.HEADS)
def test_noisy_dist_dueling_step_against_float64(L, head):
    """noisy layers under the folded head: one noisy layer of its width (value and advantages share f_in), against the
    float64 twins of tests/noisy_helpers.py on the effective parameters of this train"""
    import noisy_helpers as NH
    from xingtian_amd.model.hip_net import HipActorCritic
    a, n, b = 2, 5, 5
    spec, ospec = U.spec_pair(head, "mlp", a, n, hidden=8, noisy=True)
    assert [nl.N for nl in spec.noisy_layers] == [8, (a + 1) * n]
    net, target = HipActorCritic(spec, max_batch=8, seed=0), HipActorCritic(spec, max_batch=8, seed=0)
    net.set_weights(NH.step_weights(spec, ospec, 1, False))
    target.set_weights(NH.step_weights(spec, ospec, 2, False))
    for x in (net, target):
        x.set_noisy(NH.STEP_SEED, 0.5)
        _mark(x, head, n)
    ring = _filled_replay("mlp", net, a, 1)
    _, _, cur, nxt = U.ring_rows("mlp", a)
    net.compose(NH.STEP_CALL, 0)
    target.compose(NH.STEP_CALL, 1)
    torch.cuda.synchronize()
    host = lambda x: x.detach().cpu().numpy()
    noise, t_noise = host(net.noise).copy(), host(target.noise).copy()
    p_on = NH.oracle_params(spec, ospec, NH.effective64(spec, host(net.params), noise))
    p_tg = NH.oracle_params(spec, ospec, NH.effective64(spec, host(target.params), t_noise))
    ok = U.ok_slots(head, "mlp", a, n, ospec, p_on, p_on, None)
    assert len(ok) >= 2 * b, len(ok)
    slots = np.random.default_rng(5).permutation(ok)[:b]
    store_before = net.params.clone()
    out = net.dqn_step(target, ring.cur_state, ring.next_state, torch.from_numpy(slots).cuda(), ring.action, ring.reward,
                       ring.done, GAMMA, False, True, **_kw(head))
    net.noisy_grads()
    torch.cuda.synchronize()
    act, rew, done = (host(x)[slots] for x in (ring.action, ring.reward, ring.done))
    ref = U.DuelOracle(head, ospec, p_on, p_tg, a, n, True, 3e-4).step(cur[slots], nxt[slots], act, rew, np.full(b, GAMMA), done)
    NH.assert_step(float(host(out)[0]), net.grads_dict(), ref, spec, ospec, noise, "duel %s" % head)
    assert torch.equal(net.params, store_before) and not bool(target.grads.any())


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("head", U.HEADS)
def test_duel_mark_and_step_refusals_launch_nothing(L, head):
    from xingtian_amd.model import netspec
    from xingtian_amd.model.hip_net import HipActorCritic
    spec, ospec = U.spec_pair(head, "mlp", 2, 51)
    net, target, _, _ = _nets(head, spec, ospec, 8, mark=False)
    ring = _filled_replay("mlp", net, 2, 1)
    slots = torch.arange(4, dtype=torch.int32, device="cuda")
    args = (ring.cur_state, ring.next_state, slots, ring.action, ring.reward, ring.done, GAMMA)
    net.grads.zero_()
    with pytest.raises(RuntimeError, match="xt_net_set_duel: the net is not marked"):       # an unmarked net
        net.set_duel(True)
    _mark(net, head, 51)
    _mark(target, head, 51, duel=False)
    with pytest.raises(RuntimeError, match="same dueling mark \\(xt_net_set_duel: net 1, target_net 0\\)"):
        net.dqn_step(target, *args, False, False, **_kw(head))
    target.set_duel(True)
    with pytest.raises(RuntimeError, match="no dueling stream with a"):                     # cfg.dueling stays refused
        net.dqn_step(target, *args, True, False, **_kw(head))
    # clearing the distributional / quantile mark clears the dueling one
    _mark(target, head, 1, duel=False)
    _mark(target, head, 51, duel=False)
    with pytest.raises(RuntimeError, match="same dueling mark"):
        net.dqn_step(target, *args, False, False, **_kw(head))
    # a head of one group has no room for the value stream; 64 actions are one too many
    one = HipActorCritic(netspec.dqn_mlp((4,), 51, 8, 1), max_batch=4, seed=0)
    _mark(one, head, 51, duel=False)
    with pytest.raises(RuntimeError, match="one group of 51"):
        one.set_duel(True)
    big = HipActorCritic(netspec.dqn_mlp((4,), 65 * 2, 8, 1), max_batch=4, seed=0)
    _mark(big, head, 2, duel=False)
    with pytest.raises(RuntimeError, match="64 actions exceeds 63"):
        big.set_duel(True)
    torch.cuda.synchronize()
    assert not bool(net.grads.any())                          # nothing was launched
    target.set_duel(True)
    net.dqn_step(target, *args, False, False, **_kw(head))
    torch.cuda.synchronize()
    assert bool(net.grads.any())


# ------------------------------------------------------------------------------------------------ through the plugin pair
@pytest.mark.parametrize("head", U.HEADS)
def test_dqn_algorithm_with_dist_dueling_three_trains_against_the_oracle(L, head):
    from xingtian_amd.algorithm import alg_builder
    a_dim, n, batch = 2, 51, 32
    mc = {"dist_dueling": True, "SEED": 3, "LR": 3e-4, "HIDDEN_SIZE": 32, "NUM_LAYERS": 1}
    mc.update({"atoms": n} if head == "c51" else {"quantiles": n})
    info = {"actor": {"model_name": "DqnMlp", "type": "learner", "state_dim": [4], "action_dim": a_dim, "model_config": mc}}
    cfg = {"instance_num": 1, "agent_num": 1, "prepare_times_per_train": 1, "BUFFER_SIZE": CAP, "BATCH_SIZE": batch,
           "TARGET_UPDATE_FREQ": 2, "GAMMA": GAMMA, "double_dqn": False}
    alg = alg_builder("DQN", info, cfg)
    assert alg.device_step and alg.actor.dist_dueling and alg.actor.net.duel and alg.target_actor.net.duel
    spec, ospec = U.spec_pair(head, "mlp", a_dim, n)
    assert list(alg.actor.net.spec.names.items()) == list(spec.names.items())
    msgs, store, cur, nxt = U.ring_rows("mlp", a_dim)
    for m in msgs:
        alg.prepare_data(m)
    p_on, p_tg = H.seeded_params(ospec, 1, False), H.seeded_params(ospec, 2, False)
    alg.actor.set_weights(H.to_keras_names(spec, ospec, p_on))
    alg.target_actor.set_weights(H.to_keras_names(spec, ospec, p_tg))
    net, buf = alg.actor.net, alg.buff
    net.lib = N.CountingLib(net.lib)
    copy = lambda p: {k: v.copy() for k, v in p.items()}
    orc = U.DuelOracle(head, ospec, copy(p_on), copy(p_tg), a_dim, n, False, 3e-4)
    rng = np.random.default_rng(17)
    first = rng.permutation(U.ok_slots(head, "mlp", a_dim, n, ospec, p_on, p_tg, "target"))[:batch].tolist()
    target_init = alg.target_actor.net.params.clone()
    h = lambda x: x.cpu().numpy()
    for t in range(1, 4):
        slots = np.asarray(first if t == 1 else buf.slots_of(rng.permutation(CAP)[:batch]))
        loss = alg.train_on_slots(slots.tolist())
        batch_args = (cur[slots], nxt[slots], h(buf.action)[slots], h(buf.reward)[slots], np.full(batch, GAMMA),
                      h(buf.done)[slots])
        if t == 1:
            U.assert_step(loss, net.grads_dict(), orc.step(*batch_args), spec, ospec, "plugin train 1 " + head)
        ref = orc.step(*batch_args, apply=True)
        print("duel train", head, t, "loss", loss, float(ref["loss"]))
        assert abs(loss - ref["loss"]) <= 1e-4 * max(1.0, abs(ref["loss"])), (t, loss, ref["loss"])
        if t % 2 == 0:
            orc.sync_target()
        tp = alg.target_actor.net.params
        assert torch.equal(tp, target_init) if t < 2 else (torch.equal(tp, alg.actor.net.params) == (t == 2))
    assert alg.train_count == 3 and alg.actor.iterations == 3
    calls = net.lib.calls
    assert calls["xt_net_dqn_step_dist" if head == "c51" else "xt_net_dqn_step_quant"] == 3 and calls["xt_net_dqn_step"] == 0
    q = alg.actor.predict(cur[:9])
    assert q.shape == (9, a_dim) and q.dtype == np.float32
    want = orc.predict(cur[:9])
    assert np.abs(q - want).max() <= 1e-4 * (U.V_MAX - U.V_MIN if head == "c51" else max(1.0, np.abs(want).max()))
